"""A float32 numpy model of the prefill of include/pt_fill.h, written from the header's text on top of the models of the filters it feeds
(tests/_guided_model.py, tests/_demod_model.py) (not a test module: the helpers of tests/test_fill_abi.py and tests/test_gpu_fill.py)."""
import numpy as np

from _demod_model import demodulate, denoise_guided_demod
from _denoise_model import H5, _inv, classify
from _guided_model import _shift, denoise_guided

f32 = np.float32
CUT = f32(1e-30)


def lattice(H, W, stride, phase_x, phase_y):
    """the (H, W) bool mask of pt_render_interleaved, FRAME order"""
    yy, xx = np.mgrid[0:H, 0:W]
    return (xx % stride == phase_x) & (yy % stride == phase_y)


def fill_frame(frame, feat, sigma_normal, sigma_depth, sigma_albedo, floor=0.0, detail=False):
    """(FRAME', n_filled); detail: also a dict of hole (the holes), filled (those that found a source) and margin (the smallest factor by which a
    tap weight of a hole misses the 1e-30 cut, from either side; +inf without taps)"""
    frame = np.asarray(frame, f32)
    feat = np.asarray(feat, f32)
    A = frame[..., 3]
    hitcode = np.ascontiguousarray(feat[..., 7]).view(np.int32) >= 0
    mat = np.ascontiguousarray(feat[..., 11]).view(np.int32)
    t, Nn, Kd = feat[..., 0], feat[..., 1:4], feat[..., 4:7]
    if floor > 0:
        d = demodulate(frame, feat, np.zeros_like(frame), floor)
        x, cls = d["I"], d["cls"]
    else:
        x, cls = classify(frame, feat)
    with np.errstate(all="ignore"):
        hole = (A <= 0) & np.isfinite(feat[..., 0:7]).all(-1)
        want = np.where(hitcode, 1, 2)                                    # the class a source must have
        invN, invD, invA = _inv(1, sigma_normal), _inv(1, sigma_depth), _inv(1, sigma_albedo)
        num = np.zeros(x.shape, f32); S = np.zeros(A.shape, f32); B = np.zeros(A.shape, f32)
        found = np.zeros(A.shape, bool)
        margin = np.full(A.shape, np.inf)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dy == 0 and dx == 0:
                    continue
                use = hole & (_shift(cls, dy, dx, 0) == want) & (~hitcode | (_shift(mat, dy, dx, -1) == mat))
                dt = (t - _shift(t, dy, dx, f32(0))) / t
                e = ((Nn - _shift(Nn, dy, dx, f32(0))) ** 2).sum(-1, dtype=f32) * invN + (dt * dt) * invD + \
                    ((Kd - _shift(Kd, dy, dx, f32(0))) ** 2).sum(-1, dtype=f32) * invA
                hh = H5[dy + 2] * H5[dx + 2]
                w = np.where(hitcode, hh * np.exp(-e).astype(f32), hh).astype(f32)
                ratio = w.astype(np.float64) / 1e-30
                margin = np.where(use, np.minimum(margin, np.maximum(ratio, 1.0 / np.maximum(ratio, 1e-300))), margin)
                use = use & ~(w < CUT)
                w = np.where(use, w, f32(0)).astype(f32)
                num += np.where(use[..., None], w[..., None] * _shift(x, dy, dx, f32(0)), f32(0))
                S += w
                B = np.where(use, B + (w * w) / _shift(A, dy, dx, f32(1)), B).astype(f32)
                found |= use
        xp = num / S[..., None]
        Ap = ((S * S) / B).astype(f32)
        a = np.where((hitcode & (floor > 0))[..., None], np.maximum(Kd, f32(floor)), f32(1)).astype(f32)
        rgb = ((a * xp) * Ap[..., None]).astype(f32)
    out = frame.copy()
    out[found] = np.concatenate([rgb, Ap[..., None]], -1)[found]
    n = int(found.sum())
    if detail:
        return out, n, {"hole": hole, "filled": found, "margin": margin}
    return out, n


def denoise_guided_filled(frame, feat, T, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames, floor=0.0):
    """(H, W, 4) float32: the guided filter (floor 0) or the demodulated one over FRAME', a = the real FRAME.a"""
    frame = np.asarray(frame, f32)
    filled, _ = fill_frame(frame, feat, sigma_normal, sigma_depth, sigma_albedo, floor)
    if floor > 0:
        out = denoise_guided_demod(filled, feat, T, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames, floor)
    else:
        out = denoise_guided(filled, feat, T, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames)
    out = out.copy()
    out[..., 3] = frame[..., 3]
    return out
