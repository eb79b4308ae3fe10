#!/usr/bin/env python3
"""What an animation step costs when the caller says a bending pose as blend weights per corner and a record per joint (include/pt_skin.h: the
skinned binding 3, the refit, the patch and the motion records all on the device) against pt_move_geometry fed the same skinned triangles, which
is the parent's unchanged code path.

usage: skin_bench.py                 one child process per part (timing m3, scripts/skin_probe.py c4, timing big, skin_probe.py big); everything
                                     printed is also written to profiles/r32_skin.txt (the compile's register counts are in
                                     profiles/r32_skin_compile.txt)
       skin_bench.py timing m3|big   M3 (scenes.m3_bending) with its tube tessellated to about 100 k triangles, 8 joints | the 1 002 528-triangle
                                     height field of scripts/big_scene.py in 7 bands of scripts/pose_bench.py, each corner ramped between its
                                     band's joint and the next one's

timing prints, from one run on one context with the two routes alternating: new pose -> first rendered frame at 640 x 360, best and median of 5
each with the spread of the five, and the call alone; then the interactive step motion_mark -> pose -> reproject_frame_moved -> one frame the same
way.  pt_move_geometry makes a context's poses stale, so the skin route's object is created (outside the timings) after the move route has gone
back to the rest pose."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.path.join(ROOT, "profiles", "r32_skin.txt")
W, H = 640, 360


def band_skin(parts, n_parts, slots):
    """The two tables for a part table of bands by triangle id (pose_bench.setup): a corner of a moving triangle is ramped between its band's joint p
    and joint min(p + 1, n_parts - 1) by where the triangle lies in its band; slots = 2: (p, 1 - f), (q, f); slots = 4: each of the two split in
    halves, so four records are read.  Static triangles (part -1) have no slot."""
    assert slots in (2, 4)
    parts = np.asarray(parts, np.int64)
    n = parts.size
    s = np.arange(n, dtype=np.float64) * (n_parts + 1) / n
    f = (s - np.floor(s)).astype(np.float32)
    q = np.minimum(parts + 1, n_parts - 1)
    bone = np.full((n, 3, 4), -1, np.int32)
    weight = np.zeros((n, 3, 4), np.float32)
    moving = parts >= 0
    for k in range(slots):
        share = np.float32(1.0 if slots == 2 else 0.5)
        bone[moving, :, k] = (parts if k % 2 == 0 else q)[moving, None]
        weight[moving, :, k] = (((np.float32(1.0) - f) if k % 2 == 0 else f) * share)[moving, None]
    return bone.reshape(-1), weight.reshape(-1)


def setup(which):
    """(renderer module, scenes module, the rest pose's workload, corner_bone, corner_weight, n_parts, two poses' records)"""
    if which == "m3":
        import refit_bench as RB
        pt, hostlib, renderer, scenes = RB._load()
        scenes.GPU_BVH = 0
        rest, bone, weight, X1 = scenes.m3_bending(1, W, H, n_bones=8, n_seg=224, n_around=224)
        return renderer, scenes, rest, bone, weight, 8, [X1, scenes.m3_records(rest, 2, n_bones=8)]
    if which == "m6":                                              # scripts/skin_dq_bench.py: the same tube, twisted
        import refit_bench as RB
        pt, hostlib, renderer, scenes = RB._load()
        scenes.GPU_BVH = 0
        rest, bone, weight, X1 = scenes.m6_twisting(1, W, H, n_bones=8, n_seg=224, n_around=224)
        return renderer, scenes, rest, bone, weight, 8, [X1, scenes.m6_records(rest, 2, n_bones=8)]
    import pose_bench as PB
    renderer, scenes, rest, parts, X = PB.setup(which)
    bone, weight = band_skin(parts, PB.N_PARTS, 2)
    return renderer, scenes, rest, bone, weight, PB.N_PARTS, X


def ms(x):
    return f"{x * 1e3:.1f}"


def five(xs):
    s = sorted(xs)
    return f"best {ms(s[0])} ms, median {ms(s[len(s) // 2])} ms, spread {ms(s[-1] - s[0])} ms"


def verdict(which, what, a, b):
    ba, bb = min(a), min(b)
    sp = max(max(a) - min(a), max(b) - min(b))
    return (f"{which}: {what}: move_geometry route / skin route {bb / ba:.2f} (best of 5 each); shorter by {ms(bb - ba)} ms, the larger spread of five is "
            f"{ms(sp)} ms: {'AIM MET' if bb - ba > sp else 'AIM MISSED'}")


def timing(which, blend="linear"):
    """blend: the rule of the skin route's pose ("dq": include/pt_skin_dq.h, scripts/skin_dq_bench.py)"""
    renderer, scenes, rest, bone, weight, n_parts, X = setup(which)
    n = bone.size // 12
    static = int((bone.reshape(-1, 4)[:, 0] < 0).sum())
    print(f"{which}: {n} triangles, {rest.buffers[11].size // 3} nodes, {int(rest.buffers[13][0])} roots, {n_parts} joints, {static} static corners of {3 * n}", flush=True)
    seeds = [scenes.frame_seed(f) for f in range(1, 6)]
    plan = renderer.RefitPlan(rest.buffers)
    r = renderer.Renderer(W, H)
    r.load_workload(rest); r.reset_frame()
    r.render_batch(1, seeds[:1]); r.synchronize()
    t0 = rest.buffers[3]
    probe = r.skin_create(bone, weight, n_parts, blend=blend)
    P = [probe.triangles(x) for x in X]                            # what the move_geometry route is fed
    probe.close()

    def frame(k):
        r.reset_frame(); r.render_batch(1, seeds[k:k + 1]); r.synchronize()

    assert r.move_geometry(plan, t0)[1]; frame(0)                   # the plan's map of the record order: outside the timings
    step = {"skin": [], "move_geometry": []}
    call = {"skin": [], "move_geometry": []}
    inter = {"skin": [], "move_geometry": []}
    frames, kept = {}, {}
    for _ in range(5):
        for route in ("move_geometry", "skin"):
            assert r.move_geometry(plan, t0)[1]                     # the rest pose again, for both routes
            pose = r.skin_create(bone, weight, n_parts, blend=blend) if route == "skin" else None

            def move(k):
                if route == "skin":
                    assert r.pose_geometry(pose, X[k])[1]
                else:
                    assert r.move_geometry(plan, P[k])[1]

            move(0); frame(0)                                       # (the pose's first call makes its plan's map)
            t = time.perf_counter()
            move(1)
            call[route].append(time.perf_counter() - t)
            frame(1)
            step[route].append(time.perf_counter() - t)
            frames[route] = r.read_frame().copy()
            # the interactive step: two frames in the image, then mark -> new pose -> reproject -> one frame
            r.reset_frame(); r.render_batch(1, seeds[:2]); r.synchronize()
            t = time.perf_counter()
            r.motion_mark()
            move(0)
            kept[route] = r.reproject_frame_moved()
            r.render_batch(3, seeds[2:3]); r.synchronize()
            inter[route].append(time.perf_counter() - t)
            frames[route + " interactive"] = r.read_frame().copy()
            if pose is not None:
                pose.close()
    r.close(); plan.close()
    for route in ("skin", "move_geometry"):
        print(f"{which}: new pose -> first frame ({W}x{H}), {route} route: {five(step[route])} | the call alone: {five(call[route])}", flush=True)
    print(verdict(which, "new pose -> first frame", step["skin"], step["move_geometry"]), flush=True)
    for route in ("skin", "move_geometry"):
        print(f"{which}: mark -> pose -> reproject_frame_moved -> one frame, {route} route: {five(inter[route])}", flush=True)
    print(verdict(which, "the interactive step", inter["skin"], inter["move_geometry"]), flush=True)
    same = all(np.array_equal(frames["skin" + k].view(np.uint32), frames["move_geometry" + k].view(np.uint32)) for k in ("", " interactive"))
    print(f"{which}: the two routes' frames are bit-identical: {same}; kept by the reprojection {kept['skin']} / {kept['move_geometry']}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "timing":
        timing(sys.argv[2])
    else:
        lines = []
        here = os.path.dirname(os.path.abspath(__file__))
        for script, part in (("skin_bench.py", ("timing", "m3")), ("skin_probe.py", ("c4",)), ("skin_bench.py", ("timing", "big")), ("skin_probe.py", ("big",))):
            print(f"[{script} {' '.join(part)} ...]", flush=True)
            p = subprocess.run([sys.executable, os.path.join(here, script)] + list(part), capture_output=True, text=True, timeout=900)
            for line in p.stdout.splitlines():
                print(line, flush=True)
                lines.append(line)
            if p.returncode != 0:
                print(p.stderr[-2000:], flush=True)
                sys.exit(f"{script} {' '.join(part)} ended with {p.returncode}: nothing further is started")
            if part[-1] == "c4":
                lines.append("")
        with open(OUT, "w") as f:
            f.write("scripts/skin_bench.py: an animation step said as blend weights and joint records (pt_skin_create + pt_pose_geometry) against pt_move_geometry fed the same triangles\n")
            f.write("scripts/skin_probe.py: the two statements of the skin kernel and k_pose_quads on the device (pt_debug_skin_time, pt_debug_pose_time)\n")
            f.write("MI355X (gfx950), one process per part; 640 x 360\n\n")
            f.write("\n".join(lines) + "\n")
