#!/usr/bin/env python3
"""What an animation step costs when the caller says it as morph weights and joint records (include/pt_morph.h on a skinned pose: the morphed rest
pose, the skinned binding 3, the refit and the patch all on the device) against pt_move_geometry fed the same triangles computed beforehand, which
is the parent's only route; the host-side morph that route needs is left out of its timing, which favours it.

usage: morph_bench.py                 one child process per part (timing m4, scripts/morph_probe.py c4, timing big, morph_probe.py big); everything
                                      printed is also written to profiles/r33_morph.txt (the compile's register counts are in
                                      profiles/r33_morph_compile.txt)
       morph_bench.py timing m4|big   M4 (scenes.m4_bulging) with its tube tessellated to about 100 k triangles, 8 joints, 3 ring bulges | the
                                      1 002 528-triangle height field of scripts/big_scene.py under scripts/skin_bench.py's band skin, with 4
                                      targets, each naming every fourth corner of the first half of the moving corners

timing prints, from one run on one context with the two routes alternating: new weights and records -> first rendered frame at 640 x 360, best
and median of 5 each with the spread of the five, and the call alone.  pt_move_geometry makes a context's poses stale, so the morph route's
object is created and attached (outside the timings) after the move route has gone back to the rest pose."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.path.join(ROOT, "profiles", "r33_morph.txt")
W, H = 640, 360


def setup(which):
    """(renderer module, scenes module, the rest pose's workload, corner_bone, corner_weight, n_parts, the targets, two steps' (records, weights))"""
    if which == "m4":
        import refit_bench as RB
        pt, hostlib, renderer, scenes = RB._load()
        scenes.GPU_BVH = 0
        kw = dict(n_bones=8, n_seg=224, n_around=224)
        rest, bone, weight, targets, X1, w1 = scenes.m4_bulging(1, W, H, **kw)
        return renderer, scenes, rest, bone, weight, 8, targets, [(X1, w1), (scenes.m3_records(rest, 2, n_bones=8), scenes.m4_weights(2))]
    import morph_probe as MP
    import pose_bench as PB
    import skin_bench as SB
    renderer, scenes, rest, parts, X = PB.setup(which)
    bone, weight = SB.band_skin(parts, PB.N_PARTS, 2)
    moving = np.nonzero(np.repeat(parts >= 0, 3))[0].astype(np.int64)
    half = moving[:moving.size // 2]
    targets = [(c, d) for c, d in MP.table(rest.buffers[3], half, 4)]
    targets = [(c[:c.size // 4], d[:c.size // 4]) for c, d in targets]      # each target: every fourth corner of the half (the first quarter of its sorted list)
    return renderer, scenes, rest, bone, weight, PB.N_PARTS, targets, [(X[0], np.array([0.3, 0.9, 0.0, 0.5], np.float32)), (X[1], np.array([1.0, 0.2, 0.7, 0.0], np.float32))]


def ms(x):
    return f"{x * 1e3:.1f}"


def five(xs):
    s = sorted(xs)
    return f"best {ms(s[0])} ms, median {ms(s[len(s) // 2])} ms, spread {ms(s[-1] - s[0])} ms"


def verdict(which, what, a, b):
    ba, bb = min(a), min(b)
    sp = (max(a) - min(a)) + (max(b) - min(b))
    return (f"{which}: {what}: move_geometry route / morph route {bb / ba:.2f} (best of 5 each); shorter by {ms(bb - ba)} ms, the two spreads of five sum to "
            f"{ms(sp)} ms: {'AIM MET' if bb - ba > sp else 'AIM MISSED'}")


def timing(which):
    renderer, scenes, rest, bone, weight, n_parts, targets, steps = setup(which)
    n = bone.size // 12
    entries = sum(len(c) for c, _ in targets)
    affected = np.unique(np.concatenate([c for c, _ in targets])).size
    print(f"{which}: {n} triangles, {rest.buffers[11].size // 3} nodes, {int(rest.buffers[13][0])} roots, {n_parts} joints, {len(targets)} targets, {entries} entries on "
          f"{affected} affected corners of {3 * n}", flush=True)
    seeds = [scenes.frame_seed(f) for f in range(1, 6)]
    plan = renderer.RefitPlan(rest.buffers)
    r = renderer.Renderer(W, H)
    r.load_workload(rest); r.reset_frame()
    r.render_batch(1, seeds[:1]); r.synchronize()
    t0 = rest.buffers[3]

    def morphed_pose():
        pose = r.skin_create(bone, weight, n_parts)
        pose.morph_attach(targets)
        return pose

    probe = morphed_pose()
    P = []
    for X, w in steps:                                              # what the move_geometry route is fed: computed beforehand
        probe.morph_weights(w)
        P.append(probe.triangles(X))
    probe.morph_weights(np.zeros(len(targets), np.float32))
    assert not np.array_equal(P[1], probe.triangles(steps[1][0]))  # the morph does move something
    probe.close()

    def frame(k):
        r.reset_frame(); r.render_batch(1, seeds[k:k + 1]); r.synchronize()

    assert r.move_geometry(plan, t0)[1]; frame(0)                   # the plan's map of the record order: outside the timings
    step = {"morph": [], "move_geometry": []}
    call = {"morph": [], "move_geometry": []}
    frames = {}
    for _ in range(5):
        for route in ("move_geometry", "morph"):
            assert r.move_geometry(plan, t0)[1]                     # the rest pose again, for both routes
            pose = morphed_pose() if route == "morph" else None

            def move(k):
                if route == "morph":
                    pose.morph_weights(steps[k][1])
                    assert r.pose_geometry(pose, steps[k][0])[1]
                else:
                    assert r.move_geometry(plan, P[k])[1]

            move(0); frame(0)                                       # (the pose's first call makes its plan's map)
            t = time.perf_counter()
            move(1)
            call[route].append(time.perf_counter() - t)
            frame(1)
            step[route].append(time.perf_counter() - t)
            frames[route] = r.read_frame().copy()
            if pose is not None:
                pose.close()
    r.close(); plan.close()
    for route in ("morph", "move_geometry"):
        print(f"{which}: new weights and records -> first frame ({W}x{H}), {route} route: {five(step[route])} | the call alone: {five(call[route])}", flush=True)
    print(verdict(which, "the call alone", call["morph"], call["move_geometry"]), flush=True)
    print(verdict(which, "new weights and records -> first frame", step["morph"], step["move_geometry"]), flush=True)
    a, b = frames["morph"].view(np.uint32), frames["move_geometry"].view(np.uint32)
    rows = int((a.reshape(a.shape[0], -1) != b.reshape(b.shape[0], -1)).any(axis=1).sum())
    print(f"{which}: the two routes' frames are bit-identical in every row: {rows == 0} ({rows} of {a.shape[0]} rows differ)", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "timing":
        timing(sys.argv[2])
    else:
        lines = []
        here = os.path.dirname(os.path.abspath(__file__))
        for script, part in (("morph_bench.py", ("timing", "m4")), ("morph_probe.py", ("c4",)), ("morph_bench.py", ("timing", "big")), ("morph_probe.py", ("big",))):
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
            f.write("scripts/morph_bench.py: an animation step said as morph weights and joint records (pt_morph_weights + pt_pose_geometry) against pt_move_geometry fed the same triangles\n")
            f.write("scripts/morph_probe.py: k_morph_corners and k_pose_quads on the device (pt_debug_morph_time, pt_debug_pose_time)\n")
            f.write("MI355X (gfx950), one process per part; 640 x 360\n\n")
            f.write("\n".join(lines) + "\n")
