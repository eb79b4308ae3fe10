#!/usr/bin/env python3
"""The launch of a mix (csrc/hip/pt_rig_mix.hip: k_rig_mix, timed through pt_debug_rig_mix_time) beside the rig's launches that follow it
(k_rig_level once per level of the hierarchy, through pt_debug_rig_time over the mixed locals) in the same run; the two timers alternate, three
rounds of best-of-20 each, so that the run shows its own spread.  The geometries and layers are scripts/rig_mix_bench.py's.  Per layer a joint
reads 48 bytes of a key (96 between two keys, 48 more of key 0 for an additive layer, 4 of a mask); it writes 48.

usage: rig_mix_probe.py m8|flat|chains"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts")); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(which):
    import _rig_model as RM
    import rig_bench as RB
    import rig_mix_bench as MB
    renderer, scenes, rest, make, parent, bind, clips, masks, cases = MB.setup(which)
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
    levels = int(RM.depths(parent).max())
    best = C.c_float(0.0)
    for n_layers, steps in cases.items():
        y = MB.pack(renderer, steps[0])
        l = rig.mix_locals(y).reshape(-1)
        rounds = {"mix": [], "rig": []}
        for _ in range(3):
            assert L.pt_debug_rig_mix_time(rig._h, y.ctypes.data, y.nbytes, 20, C.byref(best)) == 0, L.pt_last_error()
            rounds["mix"].append(best.value)
            assert L.pt_debug_rig_time(rig._h, l.ctypes.data, l.nbytes, 20, C.byref(best)) == 0, L.pt_last_error()
            rounds["rig"].append(best.value)
        for name, what in (("mix", f"k_rig_mix, {n_layers} layers"), ("rig", f"k_rig_level x {levels}")):
            print(f"{which} probe: {what}: best of 20, three rounds: {' / '.join(f'{v * 1e3:.1f}' for v in rounds[name])} us", flush=True)
        a, b = min(rounds["mix"]), min(rounds["rig"])
        print(f"{which} probe: {parent.size} joints, {n_layers} layers: the mix's launch / the rig's {levels} launches {a / b:.2f}", flush=True)
    rig.close(); pose.close(); r.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "m8")
