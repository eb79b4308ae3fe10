#!/usr/bin/env python3
"""What an animation step costs when the caller says its pose as per-part matrices (include/pt_pose.h: posed binding 3, refit, patch and motion
records all on the device) against pt_move_geometry fed the same posed triangles, which is the parent's unchanged code path.

usage: pose_bench.py                 one child process per part (timing c4, scripts/pose_probe.py c4, timing big, pose_probe.py big); everything printed
                                     is also written to profiles/r31_pose.txt (the compile's register counts are in profiles/r31_pose_compile.txt)
       pose_bench.py timing c4|big   100 364 triangles (C4) | the 1 002 528-triangle height field of scripts/big_scene.py: the rest poses of
                                     scripts/move_bench.py

The first eighth of the triangles (by id) is static, the rest are seven parts under small rotations with shifts.  timing prints, from one run on
one context with the two routes alternating: new pose -> first rendered frame at 640 x 360, best and median of 5 each with the spread of the
five, and the call alone; then the interactive step motion_mark -> pose -> reproject_frame_moved -> one frame the same way.  pt_move_geometry makes a
context's poses stale, so the pose route's object is created (outside the timings) after the move route has gone back to the rest pose."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.path.join(ROOT, "profiles", "r31_pose.txt")
W, H = 640, 360
N_PARTS = 7


def rotation(axis, angle, shift):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    return np.concatenate([R, np.asarray(shift, np.float64).reshape(3, 1)], axis=1)


def setup(which):
    """(renderer module, scenes module, the rest pose's workload, a part id per triangle, two poses' records)"""
    import move_bench as MB
    renderer, scenes, rest, _ = MB.poses(which, W, H)
    n = rest.buffers[3].size // 40
    parts = (np.arange(n, dtype=np.int64) * (N_PARTS + 1) // n - 1).astype(np.int32)
    rng = np.random.RandomState(4)
    X = [renderer.pose_records(np.array([rotation(rng.normal(size=3), s * rng.uniform(0.005, 0.02), s * rng.uniform(-0.01, 0.01, 3)) for _ in range(N_PARTS)]))
         for s in (1.0, 2.0)]
    return renderer, scenes, rest, parts, X


def ms(x):
    return f"{x * 1e3:.1f}"


def five(xs):
    s = sorted(xs)
    return f"best {ms(s[0])} ms, median {ms(s[len(s) // 2])} ms, spread {ms(s[-1] - s[0])} ms"


def verdict(which, what, a, b):
    ba, bb = min(a), min(b)
    sp = max(max(a) - min(a), max(b) - min(b))
    return (f"{which}: {what}: move_geometry route / pose route {bb / ba:.2f} (best of 5 each); shorter by {ms(bb - ba)} ms, the larger spread of five is "
            f"{ms(sp)} ms: {'AIM MET' if bb - ba > sp else 'AIM MISSED'}")


def timing(which):
    renderer, scenes, rest, parts, X = setup(which)
    n = parts.size
    print(f"{which}: {n} triangles, {rest.buffers[11].size // 3} nodes, {int(rest.buffers[13][0])} roots, {N_PARTS} parts, {int((parts < 0).sum())} static triangles", flush=True)
    seeds = [scenes.frame_seed(f) for f in range(1, 6)]
    plan = renderer.RefitPlan(rest.buffers)
    r = renderer.Renderer(W, H)
    r.load_workload(rest); r.reset_frame()
    r.render_batch(1, seeds[:1]); r.synchronize()
    t0 = rest.buffers[3]
    probe = r.pose_create(parts, N_PARTS)
    P = [probe.triangles(x) for x in X]                            # what the move_geometry route is fed
    probe.close()

    def frame(k):
        r.reset_frame(); r.render_batch(1, seeds[k:k + 1]); r.synchronize()

    assert r.move_geometry(plan, t0)[1]; frame(0)                   # the plan's map of the record order: outside the timings
    step = {"pose": [], "move_geometry": []}
    call = {"pose": [], "move_geometry": []}
    inter = {"pose": [], "move_geometry": []}
    settle = []
    frames, kept = {}, {}
    for _ in range(5):
        for route in ("move_geometry", "pose"):
            assert r.move_geometry(plan, t0)[1]                     # the rest pose again, for both routes
            pose = r.pose_create(parts, N_PARTS) if route == "pose" else None

            def move(k):
                if route == "pose":
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
            if route == "pose":
                t = time.perf_counter()
                pose.close()                                        # settles: the posed binding 3 and the refit binding 10 come down
                settle.append(time.perf_counter() - t)
    r.close(); plan.close()
    for route in ("pose", "move_geometry"):
        print(f"{which}: new pose -> first frame ({W}x{H}), {route} route: {five(step[route])} | the call alone: {five(call[route])}", flush=True)
    print(verdict(which, "new pose -> first frame", step["pose"], step["move_geometry"]), flush=True)
    for route in ("pose", "move_geometry"):
        print(f"{which}: mark -> pose -> reproject_frame_moved -> one frame, {route} route: {five(inter[route])}", flush=True)
    print(verdict(which, "the interactive step", inter["pose"], inter["move_geometry"]), flush=True)
    same = all(np.array_equal(frames["pose" + k].view(np.uint32), frames["move_geometry" + k].view(np.uint32)) for k in ("", " interactive"))
    print(f"{which}: the two routes' frames are bit-identical: {same}; kept by the reprojection {kept['pose']} / {kept['move_geometry']} | "
          f"a settle (pt_pose_destroy while behind: {n * 160 / 1e6:.0f} MB + {rest.buffers[10].nbytes / 1e6:.0f} MB down) {five(settle)}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "timing":
        timing(sys.argv[2])
    else:
        lines = []
        here = os.path.dirname(os.path.abspath(__file__))
        for script, part in (("pose_bench.py", ("timing", "c4")), ("pose_probe.py", ("c4",)), ("pose_bench.py", ("timing", "big")), ("pose_probe.py", ("big",))):
            print(f"[{script} {' '.join(part)} ...]", flush=True)
            p = subprocess.run([sys.executable, os.path.join(here, script)] + list(part), capture_output=True, text=True, timeout=900)
            for line in p.stdout.splitlines():
                print(line, flush=True)
                lines.append(line)
            if p.returncode != 0:
                print(p.stderr[-2000:], flush=True)
                sys.exit(f"{script} {' '.join(part)} ended with {p.returncode}: nothing further is started")
            if part[-1] == "c4" and script == "pose_probe.py":
                lines.append("")
        with open(OUT, "w") as f:
            f.write("scripts/pose_bench.py: an animation step said as per-part matrices (pt_pose_geometry) against pt_move_geometry fed the same triangles\n")
            f.write("scripts/pose_probe.py: the two statements of k_pose on the device (pt_debug_pose_time), beside the pt_pose_geometry call\n")
            f.write("MI355X (gfx950), one process per part; 640 x 360\n\n")
            f.write("\n".join(lines) + "\n")
