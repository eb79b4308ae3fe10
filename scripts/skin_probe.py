#!/usr/bin/env python3
"""The two statements of the skin kernel (csrc/hip/pt_skin.hip) timed on the device through pt_debug_skin_time: one lane per float4 (six per
triangle) against one lane per corner (three per triangle), with two slots per corner and with four, and in the same run k_pose_quads through
pt_debug_pose_time on the same geometry: the yardstick.  The geometries are scripts/pose_probe.py's.  The skin kernel moves 288 bytes per moving
triangle (96 of the rest pose, 96 of the two tables, 96 written) against the pose kernel's 192; both are reported as bytes per second.  The
records (7 x 96 bytes here) are served by the caches and are not counted.

usage: skin_probe.py c4|big"""
import ctypes as C
import os
import sys
import time

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

    def timed(call, handle, which_kernel):
        best = C.c_float(0.0)
        rc = call(handle, x.ctypes.data, x.nbytes, which_kernel, 20, C.byref(best))
        assert rc == 0, L.pt_last_error()
        return best.value

    pose = r.pose_create(parts, PB.N_PARTS)
    t = timed(L.pt_debug_pose_time, pose._h, 0)
    print(f"{which} probe: k_pose_quads (the yardstick): best of 20 launches {t * 1e3:.1f} us ({moving} moving triangles, 96 B read + 96 B written each: "
          f"{moving * 192 / (t * 1e-3) / 1e9:.0f} GB/s)", flush=True)
    pose.close()
    for slots in (2, 4):
        bone, weight = SB.band_skin(parts, PB.N_PARTS, slots)
        skin = r.skin_create(bone, weight, PB.N_PARTS)
        for which_kernel, name in ((0, "k_skin_quads (one lane per float4)"), (1, "k_skin_corners (one lane per corner)")):
            t = timed(L.pt_debug_skin_time, skin._h, which_kernel)
            print(f"{which} probe: {slots} slots, {name}: best of 20 launches {t * 1e3:.1f} us (192 B read + 96 B written per moving triangle: "
                  f"{moving * 288 / (t * 1e-3) / 1e9:.0f} GB/s)", flush=True)
        if slots == 2:
            ts = []
            for k in range(7):
                t = time.perf_counter(); r.pose_geometry(skin, X[k % 2]); ts.append(time.perf_counter() - t)
            print(f"{which} probe: seven pt_pose_geometry calls on the skin, {PB.five(ts[1:])}", flush=True)
        skin.close()
    r.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "c4")
