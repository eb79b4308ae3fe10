"""float32 model of the history validation of include/pt_validate.h: the rule, step by step, in the header's order (numpy float32 rounds every
operation as binary32, with no contraction), so that tests/test_gpu_validate.py can hold the device to it bit for bit."""
import numpy as np

from _reproject_model import overlay

f32 = np.float32


def _clamp_var(x):
    """max(x, 0) of include/pt_guided.h: x for x >= 0, 0 for x < 0, +inf for NaN"""
    return np.where(x >= 0, x, np.where(x < 0, f32(0), f32(np.inf))).astype(f32)


def _shift(a, dy, dx, fill):
    """a[y + dy, x + dx] where that lies in the image, else fill"""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[yd, xd] = a[ys, xs]
    return out


def kappa(U, V, feat, fin, radius, z_lo, z_hi, normal_tol):
    """steps 1-3: kappa per pixel, (H, W) float32.  U, V: (H, W, 4) T now and held; feat: (H, W, 16) records; fin: the current frame inputs"""
    H, W = U.shape[:2]
    U, V, feat = (np.ascontiguousarray(a, f32) for a in (U, V, feat))
    r = int(radius)
    with np.errstate(all="ignore"):
        code = feat[..., 7].copy().view(np.int32)
        mat = feat[..., 11].copy().view(np.int32)
        hit = code != -1
        N = feat[..., 1:4]
        own = (U[..., 2] >= 1) & (V[..., 2] >= 1) & np.isfinite(U[..., 0]) & np.isfinite(U[..., 1]) & np.isfinite(V[..., 0]) & np.isfinite(V[..., 1])
        S = [np.zeros((H, W), f32) for _ in range(6)]                                              # SN, QN, NN, SH, QH, NH
        src = [U[..., 0], U[..., 1], U[..., 2], V[..., 0], V[..., 1], V[..., 2]]
        for dy in range(-r, r + 1):                                                                # 2
            for dx in range(-r, r + 1):
                inside = _shift(np.ones((H, W), bool), dy, dx, False)
                qhit, qmat, qown = _shift(hit, dy, dx, False), _shift(mat, dy, dx, 0), _shift(own, dy, dx, False)
                qN = _shift(N, dy, dx, 0)
                dot = (N[..., 0] * qN[..., 0] + N[..., 1] * qN[..., 1]) + N[..., 2] * qN[..., 2]
                tap = inside & (qhit == hit) & (~hit | ((qmat == mat) & (dot >= f32(normal_tol)))) & qown
                for k in range(6):
                    S[k] = np.where(tap, S[k] + _shift(src[k], dy, dx, 0), S[k]).astype(f32)
        SN, QN, NN, SH, QH, NH = S
        one = f32(1)
        mN = SN / NN                                                                               # 3
        s2N = _clamp_var((QN - SN * mN) / (NN - one))
        mH = SH / NH
        s2H = _clamp_var((QH - SH * mH) / (NH - one))
        var = s2N / NN + s2H / NH
        d = np.abs(mN - mH)
        z = np.sqrt((d * d) / var)
        zl, zh = f32(z_lo), f32(z_hi)
        k = np.where(np.isnan(z) | (z <= zl), one, np.where(z >= zh, f32(0), (zh - z) / (zh - zl))).astype(f32)
        k = np.where((NN >= 2) & (NH >= 2), k, one)
        k = np.where(overlay(W, H, fin), one, k)                                                   # 1
    return k.astype(f32)


def merge(N, U, Hh, V, feat, fin, radius, z_lo, z_hi, normal_tol):
    """FRAME', T', kappa and the count of the pixels with H.a > 0 and kappa < 1.  N, U: FRAME and T now; Hh, V: the held ones"""
    N, U, Hh, V = (np.ascontiguousarray(a, f32) for a in (N, U, Hh, V))
    k = kappa(U, V, feat, fin, radius, z_lo, z_hi, normal_tol)
    with np.errstate(all="ignore"):
        kk = k[..., None]
        F = np.where(kk == 0, N, N + kk * Hh).astype(f32)                                          # 4
        T = np.where(kk == 0, U, U + kk * V).astype(f32)
        T[..., 3] = 0
    return F, T, k, int(((Hh[..., 3] > 0) & (k < 1)).sum())
