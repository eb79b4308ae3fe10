"""The CPU experiment the defaults of include/pt_despeckle.h rest on: the float32 model of tests/_despeckle_model.py fed with the
oracle's frames at 160 x 90.  Error: whole-image UNCLAMPED RMSE of the mean against the mean of 256 oracle frames, at 4 and at 16 accumulated
frames.  tests/test_despeckle_abi.py asserts on the default rule; run as a program it prints the whole grid."""
import numpy as np

import _despeckle_model as DM
from test_fill_abi import _accumulate, _cpu_features

f32 = np.float32
W, H = 160, 90
GRID = [(r, k, z) for r in (1, 2, 3) for k in (2.0, 3.0, 4.0) for z in (3.0, float("inf"))]
MIN_TAPS, NORMAL_TOL, MIN_LUM = 4, 0.9, 0.0
REF_FIRST, REF_FRAMES = 5001, 256


def rmse(frame, ref):
    """whole-image unclamped RMSE of frame.rgb / frame.a against ref (H, W, 3), over the pixels where both are finite"""
    with np.errstate(all="ignore"):
        img = frame[..., :3] / frame[..., 3:4]
    ok = np.isfinite(img).all(-1) & np.isfinite(ref).all(-1)
    d = img[ok].astype(np.float64) - ref[ok]
    return float(np.sqrt((d ** 2).mean()))


class Scene:
    """a scene's records, its 256-frame reference and its accumulated frames, each computed once"""

    def __init__(self, pt, oracle, name):
        self.pt, self.oracle, self.name = pt, oracle, name
        self.wl = pt.scenes.build(name, W, H)
        self.sc = oracle.Scene.from_workload(self.wl)
        self.feat = _cpu_features(oracle, self.wl)
        b = self.wl.buffers
        self.fin = {"params": b[4], "origin": b[0], "rotation": b[1], "mouse": np.array([-1.0e6, -1.0e6, 0.0], f32)}
        self._ref = None
        self._acc = {}

    def frames(self, first, n):
        if (first, n) not in self._acc:
            self._acc[(first, n)] = _accumulate(self.oracle, self.sc, W, H, [self.pt.scenes.frame_seed(f) for f in range(first, first + n)])
        return self._acc[(first, n)]

    def ref(self):
        if self._ref is None:
            fr, T = self.frames(REF_FIRST, REF_FRAMES)
            self._ref = (fr[..., :3] / fr[..., 3:4]).astype(np.float64)
        return self._ref

    def ratio(self, first, n, radius, sigmas, own_z):
        """(despeckled RMSE / raw RMSE, raw RMSE, pixels clamped) of the n frames from `first` under the rule"""
        fr, T = self.frames(first, n)
        F, _, _, _, cnt = DM.despeckle(fr, T, self.feat, self.fin, radius, sigmas, MIN_TAPS, own_z, NORMAL_TOL, MIN_LUM)
        raw = rmse(fr, self.ref())
        return rmse(F, self.ref()) / raw, raw, cnt

    def changed_at_reference(self, radius, sigmas, own_z):
        """the share of pixels the rule changes in the 256-frame image: its cost on a converged image"""
        fr, T = self.frames(REF_FIRST, REF_FRAMES)
        return DM.despeckle(fr, T, self.feat, self.fin, radius, sigmas, MIN_TAPS, own_z, NORMAL_TOL, MIN_LUM)[4] / float(W * H)


def main():
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "oracle"))
    import ptimport
    import oracle
    pt = ptimport.load()
    oracle.lib()
    for name in ("C3", "C2"):
        s = Scene(pt, oracle, name)
        for n in (4, 16):
            print(f"{name} {W}x{H}, {n} frames: raw RMSE {s.ratio(2, n, 1, 2.0, 3.0)[1]:.5f}", flush=True)
            for r, k, z in GRID:
                ratio, raw, cnt = s.ratio(2, n, r, k, z)
                print(f"  radius {r} sigmas {k:g} own_z {z:g}: ratio {ratio:.4f}, {cnt} pixels clamped", flush=True)
        for first in (102, 202, 302):                                   # other seeds: how far a ratio moves between them
            for n in (4, 16):
                for r, k, z in GRID:
                    ratio, raw, cnt = s.ratio(first, n, r, k, z)
                    print(f"  seeds from {first}, {n} frames, radius {r} sigmas {k:g} own_z {z:g}: ratio {ratio:.4f} (raw {raw:.5f}), {cnt} clamped", flush=True)
        for r, k, z in GRID:
            print(f"  256 frames, radius {r} sigmas {k:g} own_z {z:g}: {100 * s.changed_at_reference(r, k, z):.3f} % of the pixels changed", flush=True)


if __name__ == "__main__":
    main()
