#!/usr/bin/env python3
"""The launch of a solve (csrc/hip/pt_rig_ik.hip: k_rig_ik, one lane per constraint, timed through pt_debug_rig_ik_time) beside the rig's
launches around it (k_rig_level once per level of the hierarchy, through pt_debug_rig_time over the same locals) in the same run; the two
timers alternate, three rounds of best-of-20 each, so that the run shows its own spread.  The geometries, tables and goals are
scripts/rig_ik_bench.py's.  A two-bone lane reads 16 bytes of its row, 64 of its constraint and goal, 48 of a world matrix and 112 of three
locals, and writes 32.

usage: rig_ik_probe.py m9|chars"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts")); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(which):
    import _rig_model as RM
    import rig_bench as RB
    import rig_ik_bench as IB
    renderer, scenes, rest, make, parent, bind, clips, masks, layers, cons, goals = IB.setup(which)
    r = renderer.Renderer(RB.W, RB.H)
    r.load_workload(rest); r.reset_frame()
    r.render_batch(1, [scenes.frame_seed(1)]); r.synchronize()
    L = renderer.lib()
    pose = make(r)
    rig = pose.rig(parent, bind)
    for slot, (t, v) in clips.items():
        rig.mix_clip(slot, t, v)
    for slot, w in masks.items():
        rig.mask(slot, w)
    rig.ik(cons)
    l = rig.mix_locals(layers[0]).reshape(-1)                           # (goals off: the mix alone)
    rig.ik_goals(goals[0])
    levels = int(RM.depths(parent).max())
    best = C.c_float(0.0)
    rounds = {"ik": [], "rig": []}
    for _ in range(3):
        assert L.pt_debug_rig_ik_time(rig._h, l.ctypes.data, l.nbytes, 20, C.byref(best)) == 0, L.pt_last_error()
        rounds["ik"].append(best.value)
        assert L.pt_debug_rig_time(rig._h, l.ctypes.data, l.nbytes, 20, C.byref(best)) == 0, L.pt_last_error()
        rounds["rig"].append(best.value)
    for name, what in (("ik", f"k_rig_ik, {cons.size} constraints"), ("rig", f"k_rig_level x {levels}")):
        print(f"{which} probe: {what}: best of 20, three rounds: {' / '.join(f'{v * 1e3:.1f}' for v in rounds[name])} us", flush=True)
    a, b = min(rounds["ik"]), min(rounds["rig"])
    print(f"{which} probe: {parent.size} joints, {cons.size} constraints: the solve's launch / the rig's {levels} launches {a / b:.2f}", flush=True)
    rig.close(); pose.close(); r.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "m9")
