#!/usr/bin/env python3
"""What an animation step costs when its normals are recomputed on the device (include/pt_normals.h on a morphed, skinned pose: morph, skin,
normals, refit and patch without a host round trip) against pt_move_geometry fed the same triangles computed beforehand, which is the parent's
only route to recomputed normals; the host time to make those triangles is left out of its timing, which favours it.  Also the added cost of the
step: pt_pose_geometry with mode 1 against mode 0 on one pose.

usage: normals_bench.py                 one child process per part (timing m5, scripts/normals_probe.py c4, timing big, normals_probe.py big);
                                        everything printed is also written to profiles/r34_normals.txt (the compile's register counts are in
                                        profiles/r34_normals_compile.txt)
       normals_bench.py parts small|big the two parts of one size alone, printed only
       normals_bench.py timing m5|big   M5 (scenes.m5_rippling) with its tube tessellated to about 100 k triangles, 8 joints, 3 ring bulges, the
                                        side welded | scripts/morph_bench.py's 1 002 528-triangle height field, its moving corners welded by rest
                                        position

timing prints, from one run on one context with the two routes alternating: new weights and records -> first rendered frame at 640 x 360, best
and median of 5 each with the spread of the five, and the call alone.  pt_move_geometry makes a context's poses stale, so the normals route's
object is created and attached (outside the timings) after the move route has gone back to the rest pose."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.path.join(ROOT, "profiles", "r34_normals.txt")
W, H = 640, 360
PARTS = {"small": (("normals_bench.py", ("timing", "m5")), ("normals_probe.py", ("c4",))), "big": (("normals_bench.py", ("timing", "big")), ("normals_probe.py", ("big",)))}


def setup(which):
    """morph_bench.setup and the vertex ids: (..., corner_vertex, n_vertices)"""
    import morph_bench as MOB
    renderer, scenes, rest, bone, weight, n_parts, targets, steps = MOB.setup("m4" if which == "m5" else which)
    if which == "m5":
        first, n_side, _ = rest.info["tube"]
        moved = np.arange(3 * first, 3 * (first + n_side))
    else:
        moved = np.nonzero(bone.reshape(-1, 4)[:, 0] >= 0)[0]
    ids, n_vertices = scenes.weld_corners(rest.buffers[3], moved, keep_creases=which == "m5")
    return renderer, scenes, rest, bone, weight, n_parts, targets, steps, ids, n_vertices


def ms(x):
    return f"{x * 1e3:.1f}"


def five(xs):
    s = sorted(xs)
    return f"best {ms(s[0])} ms, median {ms(s[len(s) // 2])} ms, spread {ms(s[-1] - s[0])} ms"


def verdict(which, what, a, b):
    ba, bb = min(a), min(b)
    sp = (max(a) - min(a)) + (max(b) - min(b))
    return (f"{which}: {what}: move_geometry route / normals route {bb / ba:.2f} (best of 5 each); shorter by {ms(bb - ba)} ms, the two spreads of five sum to "
            f"{ms(sp)} ms: {'AIM MET' if bb - ba > sp else 'AIM MISSED'}")


def timing(which):
    renderer, scenes, rest, bone, weight, n_parts, targets, steps, ids, n_vertices = setup(which)
    n = bone.size // 12
    length = np.bincount(ids[ids >= 0])
    print(f"{which}: {n} triangles, {rest.buffers[11].size // 3} nodes, {int(rest.buffers[13][0])} roots, {n_parts} joints, {len(targets)} targets, "
          f"{int((ids >= 0).sum())} corners of {3 * n} on {n_vertices} vertices (rows: median {int(np.median(length))}, longest {int(length.max())})", flush=True)
    seeds = [scenes.frame_seed(f) for f in range(1, 6)]
    plan = renderer.RefitPlan(rest.buffers)
    r = renderer.Renderer(W, H)
    r.load_workload(rest); r.reset_frame()
    r.render_batch(1, seeds[:1]); r.synchronize()
    t0 = rest.buffers[3]

    def normals_pose():
        pose = r.skin_create(bone, weight, n_parts)
        pose.morph_attach(targets)
        pose.normals_attach(ids, n_vertices)
        return pose

    probe = normals_pose()
    P = []
    for X, w in steps:                                              # what the move_geometry route is fed: computed beforehand
        probe.morph_weights(w)
        P.append(probe.triangles(X))
    probe.normals_mode(0)
    assert not np.array_equal(P[1], probe.triangles(steps[1][0]))  # the step does change normals
    probe.close()

    def frame(k):
        r.reset_frame(); r.render_batch(1, seeds[k:k + 1]); r.synchronize()

    assert r.move_geometry(plan, t0)[1]; frame(0)                   # the plan's map of the record order: outside the timings
    step = {"normals": [], "move_geometry": []}
    call = {"normals": [], "move_geometry": []}
    frames = {}
    for _ in range(5):
        for route in ("move_geometry", "normals"):
            assert r.move_geometry(plan, t0)[1]                     # the rest pose again, for both routes
            pose = normals_pose() if route == "normals" else None

            def move(k):
                if route == "normals":
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
    for route in ("normals", "move_geometry"):
        print(f"{which}: new weights and records -> first frame ({W}x{H}), {route} route: {five(step[route])} | the call alone: {five(call[route])}", flush=True)
    print(verdict(which, "the call alone", call["normals"], call["move_geometry"]), flush=True)
    print(verdict(which, "new weights and records -> first frame", step["normals"], step["move_geometry"]), flush=True)
    a, b = frames["normals"].view(np.uint32), frames["move_geometry"].view(np.uint32)
    rows = int((a.reshape(a.shape[0], -1) != b.reshape(b.shape[0], -1)).any(axis=1).sum())
    print(f"{which}: the two routes' frames are bit-identical in every row: {rows == 0} ({rows} of {a.shape[0]} rows differ)", flush=True)

    # the added cost of the step: the two modes alternating on one pose, the call alone
    assert r.move_geometry(plan, t0)[1]
    pose = normals_pose()
    mode = {0: [], 1: []}
    for k in range(6):
        for on in (0, 1):
            pose.normals_mode(on)
            pose.morph_weights(steps[k % 2][1])
            t = time.perf_counter()
            assert r.pose_geometry(pose, steps[k % 2][0])[1]
            if k:                                                   # (the first round makes the plan's map)
                mode[on].append(time.perf_counter() - t)
    pose.close()
    us = lambda xs: f"best {min(xs) * 1e6:.0f} us, median {sorted(xs)[len(xs) // 2] * 1e6:.0f} us, spread {(max(xs) - min(xs)) * 1e6:.0f} us"
    print(f"{which}: pt_pose_geometry, the call alone, mode 1 (recomputed): {us(mode[1])} | mode 0 (the rule's normals): {us(mode[0])} | "
          f"added by the step: {(min(mode[1]) - min(mode[0])) * 1e6:.0f} us (best against best; measured, no bound set)", flush=True)
    r.close(); plan.close()


def run(parts, lines):
    here = os.path.dirname(os.path.abspath(__file__))
    for script, part in parts:
        print(f"[{script} {' '.join(part)} ...]", flush=True)
        p = subprocess.run([sys.executable, os.path.join(here, script)] + list(part), capture_output=True, text=True, timeout=900)
        for line in p.stdout.splitlines():
            print(line, flush=True)
            lines.append(line)
        if p.returncode != 0:
            print(p.stderr[-2000:], flush=True)
            sys.exit(f"{script} {' '.join(part)} ended with {p.returncode}: nothing further is started")
        lines.append("")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "timing":
        timing(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "parts":
        run(PARTS[sys.argv[2]], [])
    else:
        lines = []
        run(PARTS["small"] + PARTS["big"], lines)
        with open(OUT, "w") as f:
            f.write("scripts/normals_bench.py: an animation step with recomputed normals (pt_normals_attach + pt_pose_geometry) against pt_move_geometry fed the same triangles\n")
            f.write("scripts/normals_probe.py: k_normals_faces + either gather and k_pose_quads on the device (pt_debug_normals_time, pt_debug_pose_time)\n")
            f.write("MI355X (gfx950), one process per part; 640 x 360\n\n")
            f.write("\n".join(lines) + "\n")
