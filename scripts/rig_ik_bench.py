#!/usr/bin/env python3
"""What an animation step costs when a mixed pose must also meet goals in world space, said as goals on the rig (include/pt_rig_ik.h:
pt_rig_ik_goals, then pt_rig_mix_pose_geometry, which solves between the mix and the levels on the device) against the route a caller has
without it: the mixed locals downloaded (pt_rig_mix_locals), the hierarchy walked and the constraints solved in C++ on one host core
(scripts/micro/rig_ik_host.cpp: the world matrices alone, then ptp::rigIk — the same locals bit for bit) and all locals uploaded again through
pt_rig_pose_geometry.  Both routes run on one context and one rig, alternating, two steps in turn.

usage: rig_ik_bench.py                one child process per part (timing m9, timing chars, scripts/rig_ik_probe.py for each, host); everything
                                      printed is also written to profiles/r38_rig_ik.txt
       rig_ik_bench.py timing m9      M9 (scenes.m9_reaching): 5 joints in one chain over M3's tube under the linear skin, one two-bone chain with a pole
       rig_ik_bench.py timing chars   C4's 100 364 triangles as 65536 rigid parts: 4096 sixteen-joint characters, four two-bone chains each
       rig_ik_bench.py host           no device: scripts/micro/rig_ik_host.cpp as a program — the walk and the solve alone over the same 65536 joints

timing prints: new goals and layers -> first rendered frame at 640 x 360, best and median of 5 each with the spread of the five; the call
alone; and the host route's three parts (download, walk and solve, upload and call)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts")); sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "r38_rig_ik.txt")
f32 = np.float32
CHARACTER = np.array([-1, 0, 1, 2, 2, 4, 5, 2, 7, 8, 0, 10, 11, 0, 13, 14], np.int32)      # hips, spine, chest, head; two arms on the chest, two legs on the hips
TIPS = (6, 9, 12, 15)
SRC = os.path.join(ROOT, "scripts", "micro", "rig_ik_host.cpp")


def host_lib(tmp):
    so = os.path.join(tmp, "rig_ik_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.rig_ik_host.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.rig_ik_host.restype = C.c_float
    return lib


def host_alone():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "rig_ik_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DRIG_IK_HOST_MAIN", "-o", exe, SRC])
        print(subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout, end="", flush=True)


def setup(which):
    """(renderer module, scenes module, the rest pose's workload, make(r) -> pose, parent, inv_bind, clips, masks, two steps' layers (packed),
    the constraints (packed), two steps' goals (packed))"""
    import rig_bench as RB
    import ptimport
    pt = ptimport.load()
    from pathtracer_0_amd import renderer
    if which == "m9":
        wl, bone, weight, parent, bind, clips, mask, _, cons, _ = pt.scenes.m9_reaching(0, RB.W, RB.H)
        layers = [renderer.rig_layers(pt.scenes.m8_layers(s)) for s in (3, 7)]
        goals = [renderer.rig_ik_goals(pt.scenes.m9_goals(wl, s)) for s in (3, 7)]
        return renderer, pt.scenes, wl, (lambda r: r.skin_create(bone, weight, parent.size)), parent, bind, {0: clips[0], 1: clips[1]}, {0: mask}, layers, renderer.rig_ik_constraints(cons), goals
    import move_bench as MB
    _, scenes, rest, _ = MB.poses("c4", RB.W, RB.H)
    n, per = RB.N_DEBRIS, CHARACTER.size
    tris = rest.buffers[3].size // 40
    parts = (np.arange(tris, dtype=np.int64) * n // tris).astype(np.int32)
    base = (np.arange(n) // per * per).astype(np.int32)
    parent = np.where(np.tile(CHARACTER, n // per) < 0, -1, base + np.tile(CHARACTER, n // per)).astype(np.int32)
    amount = 0.004 / 4
    times = np.array([0.0, 1.0, 2.5], f32)
    clips = {c: (times, np.stack([RB.small_locals(n, 10 * c + k, amount) for k in range(3)])) for c in (0, 1)}
    masks = {0: ((np.arange(n) % 16) / 15.0).astype(f32)}
    layers = [renderer.rig_layers([dict(clip=0, t=0.3 + 0.37 * s, wrap="loop"), dict(clip=1, t=0.2 + 0.29 * s, weight=0.75, mask=0, wrap="loop")]) for s in (1, 2)]
    tips = (base[::per, None] + np.array(TIPS)[None, :]).reshape(-1)
    cons = renderer.rig_ik_constraints([("two_bone", int(t), True) for t in tips])
    goals = []
    for s in (1, 2):                                                    # a small weight: the parts are debris of one room, and a full solve would throw them about
        rng = np.random.RandomState(s)
        g = np.zeros(tips.size, renderer.RIG_IK_GOAL)
        g["target"] = rng.uniform(-0.01, 0.01, (tips.size, 3)); g["pole"] = rng.uniform(-1.0, 1.0, (tips.size, 3)); g["weight"] = 0.02
        goals.append(g)
    return renderer, scenes, rest, (lambda r: r.pose_create(parts, n)), parent, None, clips, masks, layers, cons, goals


def timing(which):
    import _rig_model as RM
    import rig_bench as RB
    ms, five, W, H = RB.ms, RB.five, RB.W, RB.H
    renderer, scenes, rest, make, parent, bind, clips, masks, layers, cons, goals = setup(which)
    n = parent.size
    print(f"{which}: {rest.buffers[3].size // 40} triangles, {n} joints, depth {int(RM.depths(parent).max())}, {int((parent < 0).sum())} roots, {cons.size} constraints", flush=True)
    seeds = [scenes.frame_seed(f) for f in range(1, 6)]
    r = renderer.Renderer(W, H)
    r.load_workload(rest); r.reset_frame()
    r.render_batch(1, seeds[:1]); r.synchronize()
    pose = make(r)
    rig = pose.rig(parent, bind)
    for slot, (t, v) in clips.items():
        rig.mix_clip(slot, t, v)
    for slot, w in masks.items():
        rig.mask(slot, w)
    rig.ik(cons)
    tmp = tempfile.TemporaryDirectory()
    host = host_lib(tmp.name)

    def frame(k):
        r.reset_frame(); r.render_batch(1, seeds[k:k + 1]); r.synchronize()

    def device_route(k):
        rig.ik_goals(goals[k])
        return rig.mix(layers[k])[1]

    def host_route(k, parts=None):
        t0 = time.perf_counter()
        rig.ik_goals(None)
        l = rig.mix_locals(layers[k])                                   # downloaded
        t1 = time.perf_counter()
        host.rig_ik_host(parent.ctypes.data, n, cons.ctypes.data, goals[k].ctypes.data, cons.size, l.ctypes.data)
        t2 = time.perf_counter()
        ok = rig.pose(l)[1]                                             # uploaded, all of them
        if parts is not None:
            parts.append((t1 - t0, t2 - t1, time.perf_counter() - t2))
        return ok, l

    for k in (0, 1):                                                    # both routes and both steps once, outside the timings; and the same bits
        ok, l = host_route(k)
        rig.ik_goals(goals[k])
        assert np.array_equal(rig.ik_locals(rig.mix_locals(layers[k])).view(np.uint32), l.view(np.uint32)), "the device's solved locals are not the host's"
        assert ok and device_route(k)
        frame(k)
    step, call, parts, frames = {"ik": [], "host": []}, {"ik": [], "host": []}, [], {}
    for i in range(5):
        for route in ("host", "ik"):
            k = i % 2
            assert device_route(1 - k); frame(0)                        # the other step first, for both routes
            t = time.perf_counter()
            assert device_route(k) if route == "ik" else host_route(k, parts)[0]
            call[route].append(time.perf_counter() - t)
            frame(1)
            step[route].append(time.perf_counter() - t)
            frames[(route, k)] = r.read_frame().copy()
    for route, what in (("ik", "pt_rig_ik_goals + pt_rig_mix_pose_geometry"), ("host", "pt_rig_mix_locals + C++ walk and solve + pt_rig_pose_geometry")):
        print(f"{which}: new goals -> first frame ({W}x{H}), {route} route ({what}): {five(step[route])} | the call alone: {five(call[route])}", flush=True)
    for name, xs in zip(("the download of the mixed locals", "the walk and the solve (C++, one core)", "the upload and the call"), zip(*parts)):
        print(f"{which}: the host route's parts: {name}: {five(xs)}", flush=True)
    a, b = min(call["ik"]), min(call["host"])
    sp = max(max(v) - min(v) for v in call.values())
    print(f"{which}: the call alone, host route / device route {b / a:.2f} (best of 5 each); the difference {ms(b - a)} ms against the larger spread of five {ms(sp)} ms: "
          f"{'the device route pays' if b - a > sp else 'the device route does not pay beyond the spread' if abs(b - a) <= sp else 'the host route is shorter'}", flush=True)
    same = all(np.array_equal(frames[("ik", k)].view(np.uint32), frames[("host", k)].view(np.uint32)) for k in (0, 1))
    assert same, "the two routes' frames differ"
    print(f"{which}: the two routes' frames are bit-identical: {same}", flush=True)
    rig.close(); pose.close(); r.close()
    tmp.cleanup()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "timing":
        timing(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "host":
        host_alone()
    else:
        lines = []
        here = os.path.dirname(os.path.abspath(__file__))
        for script, part in (("rig_ik_bench.py", ("timing", "m9")), ("rig_ik_probe.py", ("m9",)), ("rig_ik_bench.py", ("timing", "chars")), ("rig_ik_probe.py", ("chars",)),
                             ("rig_ik_bench.py", ("host",))):
            print(f"[{script} {' '.join(part)} ...]", flush=True)
            p = subprocess.run([sys.executable, os.path.join(here, script)] + list(part), capture_output=True, text=True, timeout=420)
            for line in p.stdout.splitlines():
                print(line, flush=True)
                lines.append(line)
            if p.returncode != 0:
                print(p.stderr[-2000:], flush=True)
                sys.exit(f"{script} {' '.join(part)} ended with {p.returncode}: nothing further is started")
            if script == "rig_ik_probe.py":
                lines.append("")
        with open(OUT, "w") as f:
            f.write("scripts/rig_ik_bench.py: an animation step with goals in world space said as goals on the rig (pt_rig_ik_goals + pt_rig_mix_pose_geometry) against the mixed locals downloaded, "
                    "walked and solved in C++ on one core and uploaded (pt_rig_pose_geometry)\n")
            f.write("scripts/rig_ik_probe.py: the solve's launch (k_rig_ik) beside the rig's launches (k_rig_level, one per level) on the device (pt_debug_rig_ik_time, pt_debug_rig_time)\n")
            f.write("MI355X (gfx950), one process per part; 640 x 360\n\n")
            f.write("\n".join(lines) + "\n")
