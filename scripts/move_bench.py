#!/usr/bin/env python3
"""What an animation step costs with the device records patched in place (include/pt_move.h) against the move_triangles route, whose uploads of
bindings 3 and 10 make the next render lay the scene out again and upload every record array.

usage: move_bench.py                 one child process per part: timing c4, timing big, then probe c4 and probe big under a kernel trace of
                                     their own (rocprofv3 --kernel-trace --stats); everything printed is also written to profiles/r25_move.txt
       move_bench.py timing c4|big   100 352 triangles (C4 with its mesh turned) | the 1 002 528-triangle mesh of scripts/big_scene.py (rippled):
                                     the two geometries of scripts/refit_bench.py
       move_bench.py probe c4|big    a plan, a context and seven pt_move_geometry calls and nothing else timed, to run under a kernel trace

timing prints, from one run on one context: new binding 3 -> first rendered frame by the in-place route (move_geometry) and by the move_triangles
route, alternating, best and median of 5 each with the spread of the five; the call alone; and what the copies cost on their own — pt_refit_run
(binding 3 up, the refit kernels, binding 10 down) and a host copy of binding 3 (what the context's host copy costs)."""
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.path.join(ROOT, "profiles", "r25_move.txt")


def poses(which, W, H):
    import refit_bench as RB
    pt, hostlib, renderer, scenes = RB._load()
    warm = hostlib.Scene(); warm.addMaterial("m"); warm.use_gpu_bvh_builder(0)      # HIP runtime start-up outside the timings
    warm.addObjectText("o warm\nvn 0 1 0\nv 0 0 0\nv 1 0 0\nv 0 0 1\nv 1 0 1\nf 1//1 2//1 3//1\nf 2//1 4//1 3//1\n", 0)
    if which == "c4":
        scenes.GPU_BVH = 0
        rest, moved = RB.c4_pose(scenes, 0, W, H)[0], RB.c4_pose(scenes, 4, W, H)[0]
    else:
        rest, moved = RB.big_pose(hostlib, scenes, 0, W, H)[0], RB.big_pose(hostlib, scenes, 4, W, H)[0]
    assert moved.buffers[3].size == rest.buffers[3].size
    return renderer, scenes, rest, moved


def ms(x):
    return f"{x * 1e3:.1f}"


def five(xs):
    s = sorted(xs)
    return f"best {ms(s[0])} ms, median {ms(s[len(s) // 2])} ms, spread {ms(s[-1] - s[0])} ms"


def timing(which):
    W, H = 640, 360
    renderer, scenes, rest, moved = poses(which, W, H)
    n = rest.buffers[3].size // 40
    print(f"{which}: {n} triangles, {rest.buffers[11].size // 3} nodes, {int(rest.buffers[13][0])} roots", flush=True)
    seeds = [scenes.frame_seed(f) for f in range(1, 4)]
    plan = renderer.RefitPlan(rest.buffers)
    r = renderer.Renderer(W, H)
    r.load_workload(rest); r.reset_frame()
    r.render_batch(1, seeds[:1]); r.synchronize()
    a, b = rest.buffers[3], moved.buffers[3]

    def frame(k):
        r.reset_frame(); r.render_batch(1, seeds[k:k + 1]); r.synchronize()

    _, in_place = r.move_geometry(plan, a); frame(0)               # the first call makes the plan's map of the record order: outside the timings
    assert in_place
    step = {"in place": [], "move_triangles": []}
    call = {"in place": [], "move_triangles": []}
    frames = {}
    for _ in range(5):
        for route in ("in place", "move_triangles"):
            (r.move_geometry if route == "in place" else r.move_triangles)(plan, a); frame(0)      # back to the rest pose by the same route
            t = time.perf_counter()
            if route == "in place":
                assert r.move_geometry(plan, b)[1]
            else:
                r.move_triangles(plan, b)
            call[route].append(time.perf_counter() - t)
            frame(1)
            step[route].append(time.perf_counter() - t)
            frames[route] = r.read_frame().copy()
    t = time.perf_counter(); frame(2); t_next = time.perf_counter() - t
    same = bool(np.array_equal(frames["in place"].view(np.uint32), frames["move_triangles"].view(np.uint32)))
    runs, copies = [], []
    for _ in range(5):
        t = time.perf_counter(); plan.run(b); runs.append(time.perf_counter() - t)
        t = time.perf_counter(); b.copy(); copies.append(time.perf_counter() - t)
    r.close(); plan.close()
    for route in ("in place", "move_triangles"):
        print(f"{which}: new binding 3 -> first frame ({W}x{H}), {route} route: {five(step[route])} | the call alone: {five(call[route])}", flush=True)
    bi, bm = min(step["in place"]), min(step["move_triangles"])
    sp = max(max(v) - min(v) for v in step.values())
    print(f"{which}: move_triangles route / in-place route {bm / bi:.2f} (best of 5 each); shorter by {ms(bm - bi)} ms, the larger spread of five is {ms(sp)} ms: "
          f"{'AIM MET' if bm - bi > sp else 'AIM MISSED'} | the two routes' frames are bit-identical: {same} | a frame with nothing moved {ms(t_next)} ms", flush=True)
    print(f"{which}: the copies on their own: pt_refit_run ({b.nbytes / 1e6:.0f} MB up, refit, {rest.buffers[10].nbytes / 1e6:.0f} MB down) {five(runs)} | "
          f"a host copy of binding 3 {five(copies)}", flush=True)


def probe(which):
    renderer, scenes, rest, moved = poses(which, 640, 360)
    plan = renderer.RefitPlan(rest.buffers)
    r = renderer.Renderer(640, 360)
    r.load_workload(rest); r.reset_frame()
    r.render_batch(1, [scenes.frame_seed(1)]); r.synchronize()
    ts = []
    for k in range(7):
        t = time.perf_counter(); r.move_geometry(plan, (moved if k % 2 == 0 else rest).buffers[3]); ts.append(time.perf_counter() - t)
    r.close(); plan.close()
    print(f"{which} probe: seven pt_move_geometry calls, {five(ts[1:])} (under the tracer)", flush=True)


def kernel_stats(which, say):
    """the probe under a kernel trace of its own: per kernel of the refit and the patch, calls and mean duration"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "probe", which]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=d)
        for line in p.stdout.splitlines():
            if line.startswith(which):
                say(line)
        if p.returncode != 0:
            say(f"{which}: the kernel trace ended with {p.returncode}: {p.stderr[-400:]}")
            return p.returncode
        rows = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                rows += list(csv.DictReader(f))
        total = 0.0
        for row in rows:
            name = row.get("Name", "")
            if "k_move_" not in name and "k_refit_" not in name:
                continue
            calls, tot = int(row["Calls"]), float(row["TotalDurationNs"])
            total += tot / 7.0
            short = name[name.find("k_"):].split("(")[0].split("E")[0] if "k_" in name else name
            say(f"{which} kernel {short}: {calls} calls, mean {tot / calls / 1e3:.1f} us, {tot / 7.0 / 1e3:.1f} us per pt_move_geometry call")
        say(f"{which}: the kernels of one pt_move_geometry call together {total / 1e6:.3f} ms" if rows else f"{which}: no kernel statistics found")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] in ("timing", "probe"):
        (timing if sys.argv[1] == "timing" else probe)(sys.argv[2])
    else:
        lines = []

        def say(line):
            print(line, flush=True)
            lines.append(line)

        for part in (("timing", "c4"), ("timing", "big")):
            print(f"[{' '.join(part)} ...]", flush=True)
            p = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(part), capture_output=True, text=True, timeout=900)
            for line in p.stdout.splitlines():
                say(line)
            if p.returncode != 0:
                say(p.stderr[-2000:])
                sys.exit(f"move_bench.py {' '.join(part)} ended with {p.returncode}: nothing further is started")
        for which in ("c4", "big"):
            print(f"[probe {which} under the kernel trace ...]", flush=True)
            if kernel_stats(which, say) != 0:
                sys.exit(f"move_bench.py probe {which} under the kernel trace failed: nothing further is started")
        with open(OUT, "w") as f:
            f.write("scripts/move_bench.py: an animation step with the device records patched in place (pt_move_geometry) against the move_triangles route\n\n")
            f.write("\n".join(lines) + "\n")
