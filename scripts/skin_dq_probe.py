#!/usr/bin/env python3
"""The two launches of a DQ pose (csrc/hip/pt_skin_dq.hip: k_dq_records + k_skin_dq_corners, timed together through pt_debug_skin_dq_time) beside
the shipped statement of the linear skin (k_skin_corners through pt_debug_skin_time) on the same tables in the same run, with two slots per
corner and with four; the two timers alternate, three rounds of best-of-20 each, so that the run shows its own spread.  The geometries are
scripts/pose_probe.py's.  Both kernels stream 288 bytes per moving triangle (96 of the rest pose, 96 of the two tables, 96 written); the records
(7 x 96 bytes) and the table of dual quaternions (7 x 32 bytes) are served by the caches and are not counted.

usage: skin_dq_probe.py c4|big"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main(which):
    import pose_bench as PB
    import skin_bench as SB
    renderer, scenes, rest, parts, X = PB.setup(which)
    r = renderer.Renderer(PB.W, PB.H)
    r.load_workload(rest); r.reset_frame()
    r.render_batch(1, [scenes.frame_seed(1)]); r.synchronize()
    L = renderer.lib()
    x = X[1].reshape(-1)
    moving = int((parts >= 0).sum())
    best = C.c_float(0.0)
    for slots in (2, 4):
        bone, weight = SB.band_skin(parts, PB.N_PARTS, slots)
        linear = r.skin_create(bone, weight, PB.N_PARTS)
        dq = r.skin_create(bone, weight, PB.N_PARTS, blend="dq")
        rounds = {"linear": [], "dq": []}
        for _ in range(3):
            assert L.pt_debug_skin_time(linear._h, x.ctypes.data, x.nbytes, 1, 20, C.byref(best)) == 0, L.pt_last_error()
            rounds["linear"].append(best.value)
            assert L.pt_debug_skin_dq_time(dq._h, x.ctypes.data, x.nbytes, 20, C.byref(best)) == 0, L.pt_last_error()
            rounds["dq"].append(best.value)
        for name, what in (("linear", "k_skin_corners"), ("dq", "k_dq_records + k_skin_dq_corners")):
            t = min(rounds[name])
            print(f"{which} probe: {slots} slots, {what}: best of 20 launches, three rounds: {' / '.join(f'{v * 1e3:.1f}' for v in rounds[name])} us "
                  f"({moving} moving triangles, 192 B read + 96 B written each: {moving * 288 / (t * 1e-3) / 1e9:.0f} GB/s at the best)", flush=True)
        a, b = min(rounds["linear"]), min(rounds["dq"])
        spread = max(max(v) - min(v) for v in rounds.values())
        print(f"{which} probe: {slots} slots: dq / linear {b / a:.3f}; the difference {abs(b - a) * 1e3:.1f} us against the run's spread {spread * 1e3:.1f} us", flush=True)
        dq.close(); linear.close()
    r.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "c4")
