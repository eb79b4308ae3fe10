#!/usr/bin/env python3
"""The kernels of csrc/hip/pt_normals.hip timed on the device through pt_debug_normals_time — k_normals_faces plus one statement of the gather,
both statements in turn — and in the same run k_pose_quads through pt_debug_pose_time on the same geometry: the yardstick.  The geometries are
scripts/pose_probe.py's (C4's mesh, about 100 k triangles, and the 1 M height field; the first eighth static), their moving corners welded by rest
position (scenes.weld_corners).  A second table names one extra vertex at corner 0 of every hundredth moving triangle: one row of thousands of
corners among rows of about six, the known pitfall (a wave runs as long as its longest row, and rows are not split: the order of the sum is the
rule).

Bytes are counted as the statement moves them: 48 read and 16 written per listed triangle plus its 4-byte id; per walked row entry the 4-byte
corner id and the 16-byte face vector; 12 written per stored corner; the row starts (two 4-byte words per walk).  One lane per vertex walks every
row once for the sum and once more (ids only) for the stores; one lane per corner walks its vertex's whole row itself, so its entry count is the
sum of the squared row lengths, and it reads its own 4-byte row index.

usage: normals_probe.py c4|big"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
NAMES = ("one lane per vertex", "one lane per corner")


def counted_bytes(ids, statement):
    named = ids[ids >= 0]
    listed = np.unique(np.nonzero(ids >= 0)[0] // 3).size
    length = np.bincount(named)
    length = length[length > 0].astype(np.int64)
    faces = listed * (48 + 16 + 4)
    if statement == 0:
        return faces + int(length.sum()) * (4 + 16) + int(length.sum()) * (4 + 12) + length.size * 8
    return faces + int((length * length).sum()) * (4 + 16) + int(length.sum()) * (4 + 4 + 8 + 12)


def main(which):
    import pose_bench as PB
    renderer, scenes, rest, parts, X = PB.setup(which)
    r = renderer.Renderer(PB.W, PB.H)
    r.load_workload(rest); r.reset_frame()
    r.render_batch(1, [scenes.frame_seed(1)]); r.synchronize()
    L = renderer.lib()
    x = X[1].reshape(-1)
    moving_tris = int((parts >= 0).sum())
    moving = np.nonzero(np.repeat(parts >= 0, 3))[0].astype(np.int64)
    best = C.c_float(0.0)

    pose = r.pose_create(parts, PB.N_PARTS)
    assert L.pt_debug_pose_time(pose._h, x.ctypes.data, x.nbytes, 0, 20, C.byref(best)) == 0, L.pt_last_error()
    print(f"{which} probe: k_pose_quads (the yardstick): best of 20 launches {best.value * 1e3:.1f} us ({moving_tris} moving triangles, 96 B read + 96 B written each: "
          f"{moving_tris * 192 / (best.value * 1e-3) / 1e9:.0f} GB/s)", flush=True)
    pose.close()

    welded, n_vertices = scenes.weld_corners(rest.buffers[3], moving, keep_creases=False)
    fan = welded.copy()
    centre = np.nonzero(parts >= 0)[0][::100]
    fan[3 * centre] = n_vertices                                    # one vertex named by every hundredth moving triangle
    totals = [0.0, 0.0]
    for name, ids, nv in (("welded by rest position", welded, n_vertices), (f"the same with one vertex named by every hundredth moving triangle ({centre.size} corners)", fan, n_vertices + 1)):
        length = np.bincount(ids[ids >= 0])
        length = length[length > 0]
        pose = r.pose_create(parts, PB.N_PARTS)
        pose.normals_attach(ids, nv)
        for statement in (0, 1):
            assert L.pt_debug_normals_time(pose._h, x.ctypes.data, x.nbytes, statement, 20, C.byref(best)) == 0, L.pt_last_error()
            nbytes = counted_bytes(ids, statement)
            if ids is welded:
                totals[statement] += best.value
            print(f"{which} probe: k_normals_faces + the gather with {NAMES[statement]}, {name}: {int((ids >= 0).sum())} corners on {length.size} vertices "
                  f"(rows: median {int(np.median(length))}, longest {int(length.max())}): best of 20 {best.value * 1e3:.1f} us ({nbytes / 1e6:.1f} MB counted: "
                  f"{nbytes / (best.value * 1e-3) / 1e9:.0f} GB/s)", flush=True)
        pose.close()
    print(f"{which} probe: the welded table: {NAMES[0]} {totals[0] * 1e3:.1f} us, {NAMES[1]} {totals[1] * 1e3:.1f} us", flush=True)
    r.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "c4")
