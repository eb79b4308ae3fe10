"""float32 model of the outlier rejection of include/pt_despeckle.h: the rule, step by step, in the header's order (numpy float32 rounds every
operation as binary32, with no contraction), so that tests/test_gpu_despeckle.py can hold the device to it bit for bit."""
import numpy as np

from _reproject_model import overlay
from _validate_model import _clamp_var, _shift

f32 = np.float32


def _lum(c):
    return ((f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]).astype(f32)


def despeckle(frame, T, feat, fin, radius, sigmas, min_taps, own_z, normal_tol, min_lum, detail=False):
    """FRAME', T' (None when T is None), the read-only call's rgba (the rule applied to the mean, a = FRAME.a), s per pixel and the count of the
    pixels clamped.  frame, T: (H, W, 4); feat: (H, W, 16) records; fin: the current frame inputs"""
    frame, feat = np.ascontiguousarray(frame, f32), np.ascontiguousarray(feat, f32)
    T = None if T is None else np.ascontiguousarray(T, f32)
    H, W = frame.shape[:2]
    r = int(radius)
    one = f32(1)
    with np.errstate(all="ignore"):
        A = frame[..., 3]
        c = (frame[..., :3] / A[..., None]).astype(f32)
        l = _lum(c)
        measured = (A > 0) & np.isfinite(l)
        code = feat[..., 7].copy().view(np.int32)
        mat = feat[..., 11].copy().view(np.int32)
        hit = code != -1
        N = feat[..., 1:4]
        K, S, Q = (np.zeros((H, W), f32) for _ in range(3))
        for dy in range(-r, r + 1):                                                                # 2
            for dx in range(-r, r + 1):
                if dy == 0 and dx == 0:
                    continue
                inside = _shift(np.ones((H, W), bool), dy, dx, False)
                qhit, qmat, qmeas = _shift(hit, dy, dx, False), _shift(mat, dy, dx, 0), _shift(measured, dy, dx, False)
                qN, ql = _shift(N, dy, dx, 0), _shift(l, dy, dx, 0)
                dot = (N[..., 0] * qN[..., 0] + N[..., 1] * qN[..., 1]) + N[..., 2] * qN[..., 2]
                tap = inside & qmeas & (qhit == hit) & (~hit | ((qmat == mat) & (dot >= f32(normal_tol))))
                K = np.where(tap, K + one, K).astype(f32)
                S = np.where(tap, S + ql, S).astype(f32)
                Q = np.where(tap, Q + ql * ql, Q).astype(f32)
        mu = S / K                                                                                 # 4
        s2 = _clamp_var((Q - S * mu) / (K - one))
        hi = (mu + f32(sigmas) * np.sqrt(s2)).astype(f32)
        hi = np.where(hi < f32(min_lum), f32(min_lum), hi).astype(f32)
        clamp = measured & ~overlay(W, H, fin) & (K >= f32(min_taps)) & (l > hi)                   # 1, 3, 4
        if np.isfinite(f32(own_z)) and T is not None:                                              # 5
            n = T[..., 2]
            m = T[..., 0] / n
            s2p = _clamp_var((T[..., 1] - T[..., 0] * m) / (n - one))
            v = s2p / A
            d = l - mu
            oz = f32(own_z) * f32(own_z)
            clamp &= ~((n >= 2) & (d * d > oz * v))
        s = np.where(clamp, hi / l, one).astype(f32)                                               # 6
        F = frame.copy()
        F[..., :3] = np.where(clamp[..., None], frame[..., :3] * s[..., None], frame[..., :3])
        rgba = frame.copy()
        rgba[..., :3] = np.where(clamp[..., None], c * s[..., None], c)
        To = None
        if T is not None:
            scaled = np.stack([T[..., 0] * s, T[..., 1] * (s * s), T[..., 2], np.zeros((H, W), f32)], -1).astype(f32)
            To = np.where(clamp[..., None], scaled, T).astype(f32)
    if detail:
        return F, To, rgba, s, int(clamp.sum()), {"K": K, "mu": mu, "hi": hi, "l": l, "measured": measured}
    return F, To, rgba, s, int(clamp.sum())
