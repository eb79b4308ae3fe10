#!/usr/bin/env python3
"""The two statements of k_pose (csrc/hip/pt_pose.hip) timed on the device through pt_debug_pose_time: one lane per float4 (six per triangle)
against one lane per triangle, on the geometries of scripts/pose_bench.py, beside the pt_pose_geometry call they are part of.  k_move_tris, the
patch kernel that reads the same triangles, is in profiles/r25_move.txt (7.2 us at 100 k triangles, 43.7 us at 1 M).

usage: pose_probe.py c4|big"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main(which):
    import pose_bench as PB
    renderer, scenes, rest, parts, X = PB.setup(which)
    r = renderer.Renderer(PB.W, PB.H)
    r.load_workload(rest); r.reset_frame()
    r.render_batch(1, [scenes.frame_seed(1)]); r.synchronize()
    pose = r.pose_create(parts, PB.N_PARTS)
    L = renderer.lib()
    x = X[1].reshape(-1)
    moving = int((parts >= 0).sum())
    for which_kernel, name in ((0, "k_pose_quads (one lane per float4)"), (1, "k_pose_tris (one lane per triangle)")):
        best = C.c_float(0.0)
        rc = L.pt_debug_pose_time(pose._h, x.ctypes.data, x.nbytes, which_kernel, 20, C.byref(best))
        assert rc == 0, L.pt_last_error()
        gbs = moving * 2 * 96 / (best.value * 1e-3) / 1e9
        print(f"{which} probe: {name}: best of 20 launches {best.value * 1e3:.1f} us ({moving} moving triangles, 96 B read + 96 B written each: {gbs:.0f} GB/s)", flush=True)
    ts = []
    for k in range(7):
        t = time.perf_counter(); r.pose_geometry(pose, X[k % 2]); ts.append(time.perf_counter() - t)
    print(f"{which} probe: seven pt_pose_geometry calls, {PB.five(ts[1:])}", flush=True)
    pose.close(); r.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "c4")
