"""A float32 numpy model of the variance-guided filter of include/pt_guided.h, written from the header's text (not a test module: the helpers of
tests/test_guided_abi.py and tests/test_gpu_guided.py)."""
import numpy as np

from _denoise_model import H5, _inv, classify

K3 = np.array([0.25, 0.5, 0.25], np.float32)
INF32 = np.float32(np.inf)


def lum(c):
    c = np.asarray(c, np.float32)
    return (np.float32(0.2126) * c[..., 0] + np.float32(0.7152) * c[..., 1]) + np.float32(0.0722) * c[..., 2]


def _clamp_var(x):
    """max(x, 0) of the header: NaN is no estimate (+inf)"""
    return np.where(np.isnan(x), INF32, np.maximum(x, np.float32(0))).astype(np.float32)


def _shift(a, dy, dx, fill):
    """a[y + dy, x + dx] for every (y, x), `fill` outside the image"""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    if abs(dy) >= H or abs(dx) >= W:
        return out
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[yd, xd] = a[ys, xs]
    return out


def variance(frame, feat, T, min_frames):
    """v_p = s2_p / A_p of every valid pixel (0 elsewhere: never read)"""
    frame = np.asarray(frame, np.float32)
    feat = np.asarray(feat, np.float32)
    T = np.asarray(T, np.float32)
    _, cls = classify(frame, feat)
    mat = np.ascontiguousarray(feat[..., 11]).view(np.int32)
    sY, sYY, n = T[..., 0], T[..., 1], T[..., 2]
    with np.errstate(all="ignore"):
        m = sY / n
        own = _clamp_var((sYY - sY * m) / (n - np.float32(1)))
        S = np.zeros(n.shape, np.float32); Q = np.zeros(n.shape, np.float32); N = np.zeros(n.shape, np.float32)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                cq = _shift(cls, dy, dx, 0)
                use = (cq == cls) & (cls != 0) & ((cls != 1) | (_shift(mat, dy, dx, -1) == mat)) & (_shift(n, dy, dx, np.float32(0)) >= np.float32(1))
                S = np.where(use, S + _shift(sY, dy, dx, np.float32(0)), S).astype(np.float32)
                Q = np.where(use, Q + _shift(sYY, dy, dx, np.float32(0)), Q).astype(np.float32)
                N = np.where(use, N + _shift(n, dy, dx, np.float32(0)), N).astype(np.float32)
        pooled = np.where(N >= np.float32(2), _clamp_var((Q - S * (S / N)) / (N - np.float32(1))), INF32)
        s2 = np.where(n >= np.float32(min_frames), own, pooled).astype(np.float32)
        v = (s2 / frame[..., 3]).astype(np.float32)
    return np.where(cls != 0, v, np.float32(0)).astype(np.float32)


def denoise_guided(frame, feat, T, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames, return_var=False):
    """(H, W, 4) float32: rgb = the filtered mean, a = FRAME.a (and the final v when return_var)"""
    frame = np.asarray(frame, np.float32)
    feat = np.asarray(feat, np.float32)
    c, cls = classify(frame, feat)
    v = variance(frame, feat, T, min_frames)
    t, Nn, Kd = feat[..., 0], feat[..., 1:4], feat[..., 4:7]
    invN, invD, invA = _inv(1, sigma_normal), _inv(1, sigma_depth), _inv(1, sigma_albedo)
    sl = np.float32(sigma_lum)
    hitp = cls == 1
    valid = cls != 0
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            gs = np.zeros(cls.shape, np.float32); gw = np.zeros(cls.shape, np.float32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    use = valid & (_shift(cls, dy, dx, 0) == cls)
                    k = K3[dy + 1] * K3[dx + 1]
                    gs = np.where(use, gs + k * _shift(v, dy, dx, np.float32(0)), gs).astype(np.float32)
                    gw = np.where(use, gw + k, gw).astype(np.float32)
            g = gs / gw
            lum_on = np.isfinite(sl) & (g != INF32)
            den = sl * np.sqrt(g) + np.float32(1e-10)
            lp = lum(c)
            num = np.zeros(c.shape, np.float32); sw = np.zeros(cls.shape, np.float32); sv = np.zeros(cls.shape, np.float32)
            vinf = np.zeros(cls.shape, bool)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ddy, ddx = dy * s, dx * s
                    use = valid & (_shift(cls, ddy, ddx, 0) == cls)
                    cq = _shift(c, ddy, ddx, np.float32(0))
                    vq = _shift(v, ddy, ddx, np.float32(0))
                    e = np.where(lum_on, np.abs(lp - lum(cq)) / den, np.float32(0)).astype(np.float32)
                    dt = (t - _shift(t, ddy, ddx, np.float32(0))) / t
                    geo = ((Nn - _shift(Nn, ddy, ddx, np.float32(0))) ** 2).sum(-1, dtype=np.float32) * invN + (dt * dt) * invD + \
                        ((Kd - _shift(Kd, ddy, ddx, np.float32(0))) ** 2).sum(-1, dtype=np.float32) * invA
                    e = np.where(hitp, e + geo, e).astype(np.float32)
                    w = ((H5[dy + 2] * H5[dx + 2]) * np.exp(-e)).astype(np.float32)
                    use = use & ~(w < np.float32(1e-30))
                    w = np.where(use, w, np.float32(0)).astype(np.float32)
                    num += np.where(use[..., None], w[..., None] * cq, np.float32(0))
                    sw += w
                    tap_inf = use & (vq == INF32)
                    vinf |= tap_inf
                    sv = np.where(use & ~tap_inf, sv + (w * w) * vq, sv).astype(np.float32)
            c = np.where(valid[..., None], num / sw[..., None], c).astype(np.float32)
            v = np.where(valid, np.where(vinf, INF32, sv / (sw * sw)), v).astype(np.float32)
    out = np.concatenate([c, frame[..., 3:4]], axis=-1).astype(np.float32)
    return (out, v) if return_var else out
