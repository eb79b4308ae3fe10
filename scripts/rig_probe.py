#!/usr/bin/env python3
"""The launches of a rig (csrc/hip/pt_rig.hip: k_rig_level once per level of the hierarchy, timed together through pt_debug_rig_time) beside the
shipped statement of the pose rule the records then feed (k_pose_quads through pt_debug_pose_time; for M7, whose pose is skinned, k_skin_corners
through pt_debug_skin_time) in the same run; the two timers alternate, three rounds of best-of-20 each, so that the run shows its own spread.
The geometries are scripts/rig_bench.py's.  A joint reads 48 bytes of locals (and 48 of its parent's W, 48 of its inverse bind where there
is one) and writes 48 + 96.

usage: rig_probe.py m7|flat|chains"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts")); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(which):
    import _rig_model as RM
    import rig_bench as RB
    renderer, scenes, rest, make, parent, bind, locals_ = RB.setup(which)
    r = renderer.Renderer(RB.W, RB.H)
    r.load_workload(rest); r.reset_frame()
    r.render_batch(1, [scenes.frame_seed(1)]); r.synchronize()
    L = renderer.lib()
    pose = make(r)
    rig = pose.rig(parent, bind)
    l = locals_[0].reshape(-1)
    x = rig.records(locals_[0]).reshape(-1)
    levels = int(RM.depths(parent).max())
    best = C.c_float(0.0)
    rounds = {"rig": [], "rule": []}
    for _ in range(3):
        assert L.pt_debug_rig_time(rig._h, l.ctypes.data, l.nbytes, 20, C.byref(best)) == 0, L.pt_last_error()
        rounds["rig"].append(best.value)
        if which == "m7":
            assert L.pt_debug_skin_time(pose._h, x.ctypes.data, x.nbytes, 1, 20, C.byref(best)) == 0, L.pt_last_error()
        else:
            assert L.pt_debug_pose_time(pose._h, x.ctypes.data, x.nbytes, 0, 20, C.byref(best)) == 0, L.pt_last_error()
        rounds["rule"].append(best.value)
    rule = "k_skin_corners" if which == "m7" else "k_pose_quads"
    for name, what in (("rig", f"k_rig_level x {levels}"), ("rule", rule)):
        print(f"{which} probe: {what}: best of 20, three rounds: {' / '.join(f'{v * 1e3:.1f}' for v in rounds[name])} us", flush=True)
    a, b = min(rounds["rig"]), min(rounds["rule"])
    print(f"{which} probe: {parent.size} joints in {levels} launches: {a * 1e3 / levels:.1f} us per launch; the rig's launches / {rule} {a / b:.2f}", flush=True)
    rig.close(); pose.close(); r.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "m7")
