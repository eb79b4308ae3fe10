#!/usr/bin/env python3
"""What an animation step costs when the caller says its pose as local joint transforms (include/pt_rig.h: the hierarchy, the inverse binds and
the inverse transposes evaluated on the device, then pt_pose_geometry's path) against the route the parent has: the records made on the host
(tests/_rig_model.py, numpy binary32, one vectorised pass per level of the hierarchy — the same records bit for bit) and uploaded through
pt_pose_geometry.  Both routes run on one context and one pose, alternating, two sets of locals in turn.

usage: rig_bench.py                  one child process per part (timing m7, timing flat, timing chains, scripts/rig_probe.py for each); everything
                                     printed is also written to profiles/r36_rig.txt
       rig_bench.py timing m7        M7 (scenes.m7_chained): 5 joints in one chain over M3's tube under the linear skin
       rig_bench.py timing flat      C4's 100 364 triangles as 65536 rigid parts (pt_pose_create), every joint a root
       rig_bench.py timing chains    the same parts as 4096 chains of depth 16
       rig_bench.py host             no device: scripts/micro/rig_host_walk.cpp built with g++ and run — the C++ statement of the walk over the same
                                     65536 joints on one host core

timing prints: new locals -> first rendered frame at 640 x 360, best and median of 5 each with the spread of the five; the call alone; and the
host route's records alone (the numpy model; what a C++ loop takes on one core is the `host` part's figure)."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts")); sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "r36_rig.txt")
W, H = 640, 360
N_DEBRIS, DEPTH = 65536, 16
f32 = np.float32


def small_locals(n, seed, amount):
    """n locals near the identity: turns of about `amount` radians about random axes, shifts of about `amount`, no scale"""
    rng = np.random.RandomState(seed)
    l = np.zeros((n, 12), f32)
    l[:, 0:3] = rng.uniform(-amount, amount, (n, 3))
    axis = rng.normal(size=(n, 3)); axis /= np.linalg.norm(axis, axis=1)[:, None]
    half = 0.5 * rng.uniform(0.25 * amount, amount, n)
    l[:, 4:7] = axis * np.sin(half)[:, None]
    l[:, 7] = np.cos(half)
    l[:, 8:11] = 1.0
    return l


def setup(which):
    """(renderer module, scenes module, the rest pose's workload, make(r) -> pose, parent, inv_bind, two sets of locals)"""
    if which == "m7":
        import ptimport
        pt = ptimport.load()
        from pathtracer_0_amd import renderer
        wl, bone, weight, parent, bind, times, values = pt.scenes.m7_chained(W, H)
        return renderer, pt.scenes, wl, (lambda r: r.skin_create(bone, weight, parent.size)), parent, bind, [values[1], values[2]]
    import move_bench as MB
    renderer, scenes, rest, _ = MB.poses("c4", W, H)
    n = rest.buffers[3].size // 40
    parts = (np.arange(n, dtype=np.int64) * N_DEBRIS // n).astype(np.int32)
    parent = np.full(N_DEBRIS, -1, np.int32)
    if which == "chains":
        j = np.arange(N_DEBRIS)
        parent = np.where(j % DEPTH == 0, -1, j - 1).astype(np.int32)
    amount = 0.004 if which == "flat" else 0.004 / DEPTH              # (a chain's end carries the sum of its joints' motions)
    return renderer, scenes, rest, (lambda r: r.pose_create(parts, N_DEBRIS)), parent, None, [small_locals(N_DEBRIS, s, amount) for s in (1, 2)]


def host_walk():
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "rig_host_walk")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "scripts", "micro", "rig_host_walk.cpp")])
        print(subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout, end="", flush=True)


def ms(x):
    return f"{x * 1e3:.2f}"


def five(xs):
    s = sorted(xs)
    return f"best {ms(s[0])} ms, median {ms(s[len(s) // 2])} ms, spread {ms(s[-1] - s[0])} ms"


def timing(which):
    import _rig_model as RM
    renderer, scenes, rest, make, parent, bind, locals_ = setup(which)
    n_tris = rest.buffers[3].size // 40
    depth = int(RM.depths(parent).max())
    print(f"{which}: {n_tris} triangles, {parent.size} joints, depth {depth}, {int((parent < 0).sum())} roots", flush=True)
    seeds = [scenes.frame_seed(f) for f in range(1, 6)]
    r = renderer.Renderer(W, H)
    r.load_workload(rest); r.reset_frame()
    r.render_batch(1, seeds[:1]); r.synchronize()
    pose = make(r)
    rig = pose.rig(parent, bind)

    def frame(k):
        r.reset_frame(); r.render_batch(1, seeds[k:k + 1]); r.synchronize()

    for k in (0, 1):                                                   # both routes and both sets of locals once, outside the timings; and the same bits
        R = RM.records(parent, locals_[k], bind)
        assert np.array_equal(rig.records(locals_[k]).view(np.uint32), R.view(np.uint32)), "the device's records are not the model's"
        assert rig.pose(locals_[k])[1] and r.pose_geometry(pose, R)[1]
        frame(k)
    step, call, host, frames = {"rig": [], "host": []}, {"rig": [], "host": []}, [], {}
    for i in range(5):
        for route in ("host", "rig"):
            k = i % 2
            assert rig.pose(locals_[1 - k])[1]; frame(0)                # the other pose first, for both routes
            t = time.perf_counter()
            if route == "rig":
                assert rig.pose(locals_[k])[1]
            else:
                R = RM.records(parent, locals_[k], bind)
                host.append(time.perf_counter() - t)
                assert r.pose_geometry(pose, R)[1]
            call[route].append(time.perf_counter() - t)
            frame(1)
            step[route].append(time.perf_counter() - t)
            frames[(route, k)] = r.read_frame().copy()
    rig.close(); pose.close(); r.close()
    for route, what in (("rig", "pt_rig_pose_geometry"), ("host", "numpy records + pt_pose_geometry")):
        print(f"{which}: new locals -> first frame ({W}x{H}), {route} route ({what}): {five(step[route])} | the call alone: {five(call[route])}", flush=True)
    print(f"{which}: the host route's records alone (numpy, {depth} vectorised levels): {five(host)}", flush=True)
    a, b = min(call["rig"]), min(call["host"])
    sp = max(max(v) - min(v) for v in call.values())
    print(f"{which}: the call alone, host route / rig route {b / a:.2f} (best of 5 each); the difference {ms(b - a)} ms against the larger spread of five {ms(sp)} ms: "
          f"{'the device route pays' if b - a > sp else 'the device route does not pay beyond the spread' if abs(b - a) <= sp else 'the host route is shorter'}", flush=True)
    same = all(np.array_equal(frames[("rig", k)].view(np.uint32), frames[("host", k)].view(np.uint32)) for k in (0, 1))
    print(f"{which}: the two routes' frames are bit-identical: {same}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "timing":
        timing(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "host":
        host_walk()
    else:
        lines = []
        here = os.path.dirname(os.path.abspath(__file__))
        for script, part in (("rig_bench.py", ("timing", "m7")), ("rig_probe.py", ("m7",)), ("rig_bench.py", ("timing", "flat")), ("rig_probe.py", ("flat",)),
                             ("rig_bench.py", ("timing", "chains")), ("rig_probe.py", ("chains",)), ("rig_bench.py", ("host",))):
            print(f"[{script} {' '.join(part)} ...]", flush=True)
            p = subprocess.run([sys.executable, os.path.join(here, script)] + list(part), capture_output=True, text=True, timeout=420)
            for line in p.stdout.splitlines():
                print(line, flush=True)
                lines.append(line)
            if p.returncode != 0:
                print(p.stderr[-2000:], flush=True)
                sys.exit(f"{script} {' '.join(part)} ended with {p.returncode}: nothing further is started")
            if script == "rig_probe.py":
                lines.append("")
        with open(OUT, "w") as f:
            f.write("scripts/rig_bench.py: an animation step said as local joint transforms (pt_rig_pose_geometry) against the records made on the host (numpy) and pt_pose_geometry\n")
            f.write("scripts/rig_probe.py: the rig's launches (k_rig_level, one per level) beside k_pose_quads on the device (pt_debug_rig_time, pt_debug_pose_time)\n")
            f.write("MI355X (gfx950), one process per part; 640 x 360\n\n")
            f.write("\n".join(lines) + "\n")
