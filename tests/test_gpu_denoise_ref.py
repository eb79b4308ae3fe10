"""GPU: pt_denoise (include/pt_denoise.h) against the float64 reference of tests/_denoise_ref64.py, within the bound derived there: the three
injected frames of tests/test_gpu_denoise.py at 96x54 and at 1920x1080 (iterations 8: steps up to 128, taps up to 256 px away, inside the
image), and images narrower than a wave, one pixel wide or high, and around the 64 x 4 block of k_dn_pass."""
import numpy as np
import pytest

import _denoise_ref64 as ref64
from _denoise_model import denoise as model

pytestmark = pytest.mark.gpu

SIG = (0.5, 0.3, 0.05, 0.1)
INF = float("inf")


def _frames(feat, seed=5):
    """as tests/test_gpu_denoise.py at any size: random means and counts; two colours split along the hit codes; the random one with NaN,
    infinite and never-rendered pixels"""
    H, W = feat.shape[:2]
    rs = np.random.RandomState(seed)
    cnt = rs.randint(1, 9, size=(H, W, 1)).astype(np.float32)
    rnd = np.concatenate([rs.rand(H, W, 3).astype(np.float32) * cnt, cnt], -1)
    code = np.ascontiguousarray(feat[..., 7]).view(np.int32)
    two = np.zeros((H, W, 4), np.float32)
    two[..., 3] = 4.0
    two[..., :3] = np.where(((code & 1) == 1)[..., None], np.float32(3.6), np.float32(0.4))
    bad = rnd.copy()
    bad[rs.randint(H), rs.randint(W), 0] = np.nan
    bad[rs.randint(H), rs.randint(W), :3] = np.inf
    bad[rs.randint(H), rs.randint(W)] = (5.0, 6.0, 7.0, 0.0)
    return {"random": rnd, "two_colour": two, "nan_alpha0": bad}


def _ctx(pt, renderer_mod, w, h):
    r = renderer_mod.Renderer(w, h)
    r.load_workload(pt.scenes.build("C3", w, h))
    return r


def _check(r, feat, cases, with_model):
    worst = 0.0
    for fname, fr in _frames(feat).items():
        r.write_frame(fr)
        for it, sig in cases:
            got = r.denoise(it, *sig)
            want, R, M = ref64.denoise(fr, feat, it, *sig)
            dev, at = ref64.deviation(got, want, R, M, it)
            assert dev <= 1.0, (feat.shape[:2], fname, it, sig, dev, at, got[at], want[at])
            worst = max(worst, dev)
            if with_model:
                m = model(fr, feat, it, *sig)
                assert np.allclose(got, m, rtol=1e-4, atol=1e-6, equal_nan=True), (fname, it, sig, np.nanmax(np.abs(got - m)))
    return worst


def test_agrees_with_the_float64_reference_96x54(pt, renderer_mod):
    r = _ctx(pt, renderer_mod, 96, 54)
    feat = r.read_features()
    worst = _check(r, feat, [(5, SIG), (3, (0.2, 0.1, 0.02, 0.05)), (2, (INF, INF, INF, INF)), (0, SIG), (8, (1.0, INF, 0.1, INF))], True)
    r.close()
    print(f"denoise 96x54: largest deviation {worst:.4f} of the bound")


def test_agrees_with_the_float64_reference_1080p(pt, renderer_mod):
    r = _ctx(pt, renderer_mod, 1920, 1080)
    feat = r.read_features()
    worst = _check(r, feat, [(8, SIG)], False)
    r.close()
    print(f"denoise 1920x1080: largest deviation {worst:.4f} of the bound")


@pytest.mark.parametrize("w,h", [(1, 1), (1, 37), (37, 1), (63, 5), (64, 4), (65, 3), (129, 7)])
def test_edge_shapes(pt, renderer_mod, w, h):
    r = _ctx(pt, renderer_mod, w, h)
    feat = r.read_features()
    _check(r, feat, [(0, SIG), (1, SIG), (3, (0.2, 0.1, 0.02, 0.05)), (8, SIG), (8, (1.0, INF, 0.1, INF))], True)
    r.close()
