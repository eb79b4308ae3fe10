#!/usr/bin/env python3
"""What an animation step costs when the caller says its pose as layers over clips that lie on the device (include/pt_rig_mix.h: one launch of
k_rig_mix, then the rig's levels and pt_pose_geometry's path) against the route the parent has: the same locals mixed on the host
(tests/_rig_mix_model.py, numpy binary32 — the same locals bit for bit) and uploaded through pt_rig_pose_geometry.  Both routes run on one
context and one rig, alternating, two steps in turn.

usage: rig_mix_bench.py                one child process per part (timing m8, timing flat, timing chains, scripts/rig_mix_probe.py for each, host);
                                       everything printed is also written to profiles/r37_rig_mix.txt
       rig_mix_bench.py timing m8      M8 (scenes.m8_mixed): 5 joints in one chain over M3's tube under the linear skin, its 3 layers
       rig_mix_bench.py timing flat    C4's 100 364 triangles as 65536 rigid parts (pt_pose_create), every joint a root, with 2 and with 8 layers
       rig_mix_bench.py timing chains  the same parts as 4096 chains of depth 16, with 2 and with 8 layers
       rig_mix_bench.py host           no device: scripts/micro/rig_mix_host.cpp built with g++ and run — ptp::rigMix over 65536 joints on one host core

timing prints: new layers -> first rendered frame at 640 x 360, best and median of 5 each with the spread of the five; the call alone; and the
host route's mix alone (the numpy model; what a C++ loop takes on one core is the `host` part's figure).  The masks of the large cases have 16
distinct weights: the numpy model blends the joints of one weight together, so a mask of 65536 distinct weights would cost it far more."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts")); sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "r37_rig_mix.txt")
f32 = np.float32


def layers_of(n_layers, step):
    """the model's layers of a large case at `step`: the base looping between keys, then override and additive layers in turn, every one masked"""
    import _rig_mix_model as MM
    out = [MM.layer(0, 0.3 + 0.37 * step, wrap=MM.LOOP)]
    for l in range(1, n_layers):
        out.append(MM.layer(l % 2, 0.2 * l + 0.29 * step, 0.75, 0, MM.OVERRIDE if l % 2 else MM.ADDITIVE, MM.LOOP))
    return out


def setup(which):
    """(renderer module, scenes module, the rest pose's workload, make(r) -> pose, parent, inv_bind, clips, masks, {n_layers: two steps' layers})"""
    import _rig_mix_model as MM
    import rig_bench as RB
    if which == "m8":
        import ptimport
        pt = ptimport.load()
        from pathtracer_0_amd import renderer
        wl, bone, weight, parent, bind, clips, mask, _ = pt.scenes.m8_mixed(0, RB.W, RB.H)
        steps = []
        for s in (3, 7):
            y = renderer.rig_layers(pt.scenes.m8_layers(s))
            steps.append([MM.layer(int(a["clip"]), a["t"], a["weight"], int(a["mask"]), int(a["mode"]), int(a["wrap"])) for a in y])
        return renderer, pt.scenes, wl, (lambda r: r.skin_create(bone, weight, parent.size)), parent, bind, {0: clips[0], 1: clips[1]}, {0: mask}, {3: steps}
    renderer, scenes, rest, make, parent, bind, _ = RB.setup(which)
    n = parent.size
    amount = 0.004 if which == "flat" else 0.004 / RB.DEPTH
    times = np.array([0.0, 1.0, 2.5], f32)
    clips = {c: (times, np.stack([RB.small_locals(n, 10 * c + k, amount) for k in range(3)])) for c in (0, 1)}
    masks = {0: ((np.arange(n) % 16) / 15.0).astype(f32)}
    return renderer, scenes, rest, make, parent, bind, clips, masks, {k: [layers_of(k, s) for s in (1, 2)] for k in (2, 8)}


def pack(renderer, layers):
    return renderer.rig_layers([dict(clip=y["clip"], t=y["t"], weight=y["weight"], mask=y["mask"], mode=y["mode"], wrap=y["wrap"]) for y in layers])


def host_mix():
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "rig_mix_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "scripts", "micro", "rig_mix_host.cpp")])
        print(subprocess.run([exe], capture_output=True, text=True, check=True, timeout=120).stdout, end="", flush=True)


def timing(which):
    import _rig_mix_model as MM
    import _rig_model as RM
    import rig_bench as RB
    ms, five, W, H = RB.ms, RB.five, RB.W, RB.H
    renderer, scenes, rest, make, parent, bind, clips, masks, cases = setup(which)
    n = parent.size
    print(f"{which}: {rest.buffers[3].size // 40} triangles, {n} joints, depth {int(RM.depths(parent).max())}, {int((parent < 0).sum())} roots", flush=True)
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

    def frame(k):
        r.reset_frame(); r.render_batch(1, seeds[k:k + 1]); r.synchronize()

    for n_layers, steps in cases.items():
        tag = f"{which}, {n_layers} layers"
        packed = [pack(renderer, s) for s in steps]
        for k in (0, 1):                                               # both routes and both steps once, outside the timings; and the same bits
            l = MM.mix_locals(clips, masks, steps[k], n)
            assert np.array_equal(rig.mix_locals(packed[k]).view(np.uint32), l.view(np.uint32)), "the device's locals are not the model's"
            assert rig.mix(packed[k])[1] and rig.pose(l)[1]
            frame(k)
        step, call, host, frames = {"mix": [], "host": []}, {"mix": [], "host": []}, [], {}
        for i in range(5):
            for route in ("host", "mix"):
                k = i % 2
                assert rig.mix(packed[1 - k])[1]; frame(0)              # the other step first, for both routes
                t = time.perf_counter()
                if route == "mix":
                    assert rig.mix(packed[k])[1]
                else:
                    l = MM.mix_locals(clips, masks, steps[k], n)
                    host.append(time.perf_counter() - t)
                    assert rig.pose(l)[1]
                call[route].append(time.perf_counter() - t)
                frame(1)
                step[route].append(time.perf_counter() - t)
                frames[(route, k)] = r.read_frame().copy()
        for route, what in (("mix", "pt_rig_mix_pose_geometry"), ("host", "numpy mix + pt_rig_pose_geometry")):
            print(f"{tag}: new layers -> first frame ({W}x{H}), {route} route ({what}): {five(step[route])} | the call alone: {five(call[route])}", flush=True)
        print(f"{tag}: the host route's mix alone (numpy): {five(host)}", flush=True)
        a, b = min(call["mix"]), min(call["host"])
        sp = max(max(v) - min(v) for v in call.values())
        print(f"{tag}: the call alone, host route / mix route {b / a:.2f} (best of 5 each); the difference {ms(b - a)} ms against the larger spread of five {ms(sp)} ms: "
              f"{'the device route pays' if b - a > sp else 'the device route does not pay beyond the spread' if abs(b - a) <= sp else 'the host route is shorter'}", flush=True)
        same = all(np.array_equal(frames[("mix", k)].view(np.uint32), frames[("host", k)].view(np.uint32)) for k in (0, 1))
        assert same, "the two routes' frames differ"
        print(f"{tag}: the two routes' frames are bit-identical: {same}", flush=True)
    rig.close(); pose.close(); r.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "timing":
        timing(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "host":
        host_mix()
    else:
        lines = []
        here = os.path.dirname(os.path.abspath(__file__))
        for script, part in (("rig_mix_bench.py", ("timing", "m8")), ("rig_mix_probe.py", ("m8",)), ("rig_mix_bench.py", ("timing", "flat")), ("rig_mix_probe.py", ("flat",)),
                             ("rig_mix_bench.py", ("timing", "chains")), ("rig_mix_probe.py", ("chains",)), ("rig_mix_bench.py", ("host",))):
            print(f"[{script} {' '.join(part)} ...]", flush=True)
            p = subprocess.run([sys.executable, os.path.join(here, script)] + list(part), capture_output=True, text=True, timeout=420)
            for line in p.stdout.splitlines():
                print(line, flush=True)
                lines.append(line)
            if p.returncode != 0:
                print(p.stderr[-2000:], flush=True)
                sys.exit(f"{script} {' '.join(part)} ended with {p.returncode}: nothing further is started")
            if script == "rig_mix_probe.py":
                lines.append("")
        with open(OUT, "w") as f:
            f.write("scripts/rig_mix_bench.py: an animation step said as layers over clips on the device (pt_rig_mix_pose_geometry) against the same locals mixed on the host (numpy) and pt_rig_pose_geometry\n")
            f.write("scripts/rig_mix_probe.py: the mix's launch (k_rig_mix) beside the rig's launches (k_rig_level, one per level) on the device (pt_debug_rig_mix_time, pt_debug_rig_time)\n")
            f.write("MI355X (gfx950), one process per part; 640 x 360\n\n")
            f.write("\n".join(lines) + "\n")
