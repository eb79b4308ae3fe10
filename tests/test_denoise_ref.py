"""CPU: the float32 denoiser model (tests/_denoise_model.py) against the float64 reference of tests/_denoise_ref64.py, within the bound that
module derives, on synthetic frames and feature records; and the same comparison failing for models with one rule of include/pt_denoise.h
misread, so that the bound is known to be tight enough to catch such a misreading on the device (tests/test_gpu_denoise_ref.py)."""
import os
import types

import numpy as np
import pytest

import _denoise_model
import _denoise_ref64 as ref64

INF = float("inf")
SIGMAS = [(0.5, 0.3, 0.3, 0.2), (0.2, 0.1, 0.05, 0.1), (1.0, INF, 0.3, INF), (INF, INF, INF, INF)]


def synthetic(H, W, seed=1):
    """(frame, feat): random means and counts; varying depth, normals and albedo; a block of misses and scattered ones; a never-rendered
    pixel with colour, a NaN mean, an infinite one, a NaN normal, an infinite depth"""
    rs = np.random.RandomState(seed)
    cnt = rs.randint(1, 9, size=(H, W, 1)).astype(np.float32)
    frame = np.concatenate([rs.rand(H, W, 3).astype(np.float32) * cnt * np.float32(2.0), cnt], -1)
    feat = _denoise_model.features(H, W)
    feat[..., 0] = (0.5 + 2.5 * rs.rand(H, W)).astype(np.float32)
    n = rs.randn(H, W, 3).astype(np.float32) * np.float32(0.3) + np.array([0.0, 1.0, 0.0], np.float32)
    feat[..., 1:4] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    feat[..., 4:7] = np.where((np.arange(W) < W // 2)[None, :, None], np.float32(0.3), np.float32(0.7)) + rs.rand(H, W, 3).astype(np.float32) * np.float32(0.05)
    miss = rs.rand(H, W) < 0.15
    miss[: H // 3, : W // 4] = True
    code = np.where(miss, -1, 0x1000000 + (np.arange(W)[None, :] // 7)).astype(np.int32)
    feat[..., 7] = code.view(np.float32)
    feat[miss, 0] = -1.0
    feat[miss, 1:7] = 0.0
    if H > 4 and W > 6:
        frame[1, 2] = (3.0, 4.0, 5.0, 0.0)                        # never rendered
        frame[2, 3, 1] = np.nan
        frame[3, 4, :3] = np.inf
        feat[4, 5, 2] = np.nan
        feat[H - 1, W - 1, 0] = np.inf
    return frame, feat


def _worst(model, frame, feat, it, sig):
    want, R, M = ref64.denoise(frame, feat, it, *sig)
    return ref64.deviation(model(frame, feat, it, *sig), want, R, M, it)


SHAPES = [(23, 37), (1, 1), (1, 13), (13, 1), (5, 70), (40, 9)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_float32_model_within_the_bound(H, W):
    frame, feat = synthetic(H, W)
    for sig in SIGMAS:
        for it in (0, 1, 3, 6):
            worst, at = _worst(_denoise_model.denoise, frame, feat, it, sig)
            assert worst <= 1.0, (H, W, sig, it, worst, at)


def test_the_reference_on_hand_cases():
    # a single valid pixel, or iterations 0: the mean itself; an invalid pixel: its mean or, at alpha 0, its raw rgb
    frame = np.array([[[1.0, 2.0, 3.0, 4.0]]], np.float32)
    feat = _denoise_model.features(1, 1)
    for it in (0, 5):
        out, _, _ = ref64.denoise(frame, feat, it, 0.5, 0.3, 0.05, 0.1)
        assert np.array_equal(out, [[[0.25, 0.5, 0.75, 4.0]]])
    frame[0, 0, 3] = 0.0
    assert np.array_equal(ref64.denoise(frame, feat, 3, 0.5, 0.3, 0.05, 0.1)[0], [[[1.0, 2.0, 3.0, 0.0]]])
    # two pixels of one row, one pass: each is (6*c_p + 4*w*c_q) / (6 + 4*w) with w = exp(-|c_p - c_q|^2 / sc^2) (equal guides)
    frame = np.array([[[0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0]]], np.float32)
    out, _, _ = ref64.denoise(frame, _denoise_model.features(1, 2), 1, 2.0, 1.0, 1.0, 1.0)
    w = np.exp(-3.0 / 4.0)
    assert np.allclose(out[0, :, 0], [4 * w / (6 + 4 * w), (6 + 0 * w) / (6 + 4 * w)], rtol=1e-15, atol=0)
    # pass 1 (step 2) weighs the colour with sc^2 * 4^-1: pixel 0 of three takes pixel 2 at h = 4/16 beside its own 6/16
    frame = np.array([[[0.0, 0.0, 0.0, 1.0], [5.0, 5.0, 5.0, 1.0], [1.0, 1.0, 1.0, 1.0]]], np.float32)
    feat = _denoise_model.features(1, 3)
    c = ref64.denoise(frame, feat, 1, 2.0, INF, INF, INF)[0][0, :, 0]
    w = np.exp(-3.0 * (c[0] - c[2]) ** 2 / (4.0 / 4.0))
    two = ref64.denoise(frame, feat, 2, 2.0, INF, INF, INF)[0]
    assert abs(two[0, 0, 0] - (6 * c[0] + 4 * w * c[2]) / (6 + 4 * w)) < 1e-14


# one misreading of include/pt_denoise.h each, applied to the float32 model's text
MUTATIONS = {
    "no_4^-i": ("_inv(4 ** i, sigma_color)", "_inv(1, sigma_color)"),
    "clamp_out_of_image_taps": ("use = inb & (cls != 0)", "use = (cls != 0)"),
    "depth_over_t_q": ("dt = (t - t[qy, qx]) / t", "dt = (t - t[qy, qx]) / t[qy, qx]"),
    "hit_and_miss_mix": ("(cls[qy, qx] == cls)", "(cls[qy, qx] != 0)"),
    "box_instead_of_b3": ("H5 = np.array([1, 4, 6, 4, 1], np.float32) / np.float32(16)", "H5 = np.ones(5, np.float32) / np.float32(5)"),
}


def _mutant(name):
    old, new = MUTATIONS[name]
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "_denoise_model.py")).read()
    assert src.count(old) == 1, name
    mod = types.ModuleType("_denoise_mutant_" + name)
    exec(compile(src.replace(old, new), mod.__name__, "exec"), mod.__dict__)
    return mod.denoise


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutated_models_fail_the_bound(name):
    bad = _mutant(name)
    frame, feat = synthetic(23, 37)
    worst = max(_worst(bad, frame, feat, it, sig)[0] for sig in SIGMAS[:2] for it in (1, 3))
    assert worst > 1.0, (name, worst)
    # ... and by a wide margin: the bound is not the reason they fail narrowly
    assert worst > 100.0, (name, worst)
