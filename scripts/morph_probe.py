#!/usr/bin/env python3
"""k_morph_corners (csrc/hip/pt_morph.hip) timed on the device through pt_debug_morph_time, and in the same run k_pose_quads through
pt_debug_pose_time on the same geometry: the yardstick.  The geometries are scripts/pose_probe.py's (100 k and 1 M triangles, the first eighth
static).  Tables: a quarter (the first, contiguous) and all of the moving corners affected; 4 and 64 targets, every affected corner named by four
of them, with 1 / 8 / all weights non-zero; and one skewed table of 64 targets, every hundredth affected corner named by all of them and the
others by one.  Bytes are counted as 72 per affected corner (its id, its row start, 32 read and 32 written of the rest pose), 32 per entry whose
weight is not zero and 4 per skipped entry; the weights (at most 256 bytes here) are served by the caches and are not counted.  (The kernel
loads a skipped entry whole — its loads are issued before its weight is known — so its time does not fall with the number of zero weights and
the byte rate counted this way does.)

usage: morph_probe.py c4|big"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))


def table(tris, affected, n_targets, skew=False, amp=1e-3):
    """targets (a list of (corners, deltas)) over the corners `affected`: each named by four targets a quarter of n_targets apart, or — skew —
    every hundredth by all targets and the others by one.  The vertex delta runs along the corner's rest normal."""
    tris = np.asarray(tris, np.float32).reshape(-1, 40)
    i = np.arange(affected.size, dtype=np.int64)
    if skew:
        heavy = i[::100]
        corner = np.concatenate([affected[i], np.repeat(affected[heavy], n_targets - 1)])
        first = i % n_targets
        target = np.concatenate([first, ((first[heavy][:, None] + 1 + np.arange(n_targets - 1)[None, :]) % n_targets).reshape(-1)])
    else:
        corner = np.tile(affected, 4)
        target = np.concatenate([(i + s * (n_targets // 4)) % n_targets for s in range(4)])
    order = np.argsort(target, kind="stable")
    corner, target = corner[order], target[order]
    k, c = corner // 3, corner % 3
    delta = np.zeros((corner.size, 6), np.float32)
    for j in range(3):
        delta[:, j] = amp * tris[k, 12 + 4 * c + j]
    delta[~np.isfinite(delta)] = 0.0
    ends = np.concatenate([[0], np.cumsum(np.bincount(target, minlength=n_targets))])
    return [(corner[a:b].astype(np.int32), delta[a:b]) for a, b in zip(ends[:-1], ends[1:])]


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

    configs = [(share, n_targets, False) for share in ("a quarter", "all") for n_targets in (4, 64)] + [("all", 64, True)]
    for share, n_targets, skew in configs:
        affected = moving[:moving.size // 4] if share == "a quarter" else moving
        targets = table(rest.buffers[3], affected, n_targets, skew)
        pose = r.pose_create(parts, PB.N_PARTS)
        pose.morph_attach(targets)
        for nonzero in ((1, n_targets) if n_targets == 4 else (1, 8, n_targets)):
            w = np.zeros(n_targets, np.float32); w[:nonzero] = 0.5
            read = sum(len(c) for c, _ in targets[:nonzero])
            skipped = sum(len(c) for c, _ in targets[nonzero:])
            assert L.pt_debug_morph_time(pose._h, w.ctypes.data, w.nbytes, 20, C.byref(best)) == 0, L.pt_last_error()
            nbytes = 72 * affected.size + 32 * read + 4 * skipped
            name = "skewed (1 % of the corners named by all 64 targets, the others by one)" if skew else "four entries per corner"
            print(f"{which} probe: k_morph_corners, {share} of the moving corners ({affected.size}), {n_targets} targets, {name}, {nonzero} weights non-zero: "
                  f"best of 20 launches {best.value * 1e3:.1f} us ({read} entries read, {skipped} skipped, {nbytes / 1e6:.1f} MB: {nbytes / (best.value * 1e-3) / 1e9:.0f} GB/s)", flush=True)
        pose.close()
    r.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "c4")
