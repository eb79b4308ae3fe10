"""The float32 numpy model of include/pt_bloom.h, steps 0-4: what pt_bloom must equal bit for bit, and, chained with tests/_tonemap_model.py, what
pt_tonemap_bloom must.  Every array operation below is one binary32 operation per element in the header's order (numpy contracts nothing).
A rule is a dict of the struct's fields; (c, A) come from _tonemap_model.from_frame / from_image; images are (H, W, 3) arrays, row 0 first."""
import numpy as np

import _tonemap_model as TM

f32 = np.float32
RULE = dict(levels=6, intensity=0.05, threshold=1.0, spread=0.75)
SRC_FRAME, SRC_HOST, SRC_FILTERED = 0, 1, 2
W4 = (f32(0.125), f32(0.375), f32(0.375), f32(0.125))
U4 = (f32(0.5625), f32(0.1875), f32(0.1875), f32(0.0625))


def rule(**kw):
    assert not set(kw) - set(RULE)
    return dict(RULE, **kw)


def sizes(W, H, L):
    """[(W_0, H_0), ..., (W_L, H_L)]"""
    out = [(W, H)]
    for _ in range(L):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def norm(spread, L):
    p = s = f32(1.0)
    for _ in range(L - 1):
        p = f32(p * f32(spread))
        s = f32(s + p)
    return f32(f32(1.0) / s)


def threshold(rule_threshold, exposure):
    with np.errstate(all="ignore"):
        return f32(f32(rule_threshold) / f32(exposure))


def clean(c, A):
    """step 0: s of (c, A), (n, 3)"""
    with np.errstate(all="ignore"):
        s = np.where(np.isnan(c), f32(0), np.where(c < 0, f32(0), np.where(c > f32(65504.0), f32(65504.0), c))).astype(f32)
        return np.where((A > 0)[:, None], s, f32(0)).astype(f32)


def bright(s, T):
    """step 1: B of s, (n, 3)"""
    l = TM.luminance(s)
    with np.errstate(all="ignore"):
        k = np.where(l > f32(T), (l - f32(T)) / l, f32(0)).astype(f32)
    return (s * k[:, None]).astype(f32)


def _tent(p0, p1, p2, p3):
    return (W4[0] * p0 + W4[1] * p1) + (W4[2] * p2 + W4[3] * p3)


def down(V):
    """step 2: the next coarser level of V (H, W, 3)"""
    H, W = V.shape[:2]
    xs = np.clip(2 * np.arange((W + 1) // 2)[:, None] - 1 + np.arange(4), 0, W - 1)
    ys = np.clip(2 * np.arange((H + 1) // 2)[:, None] - 1 + np.arange(4), 0, H - 1)
    R = _tent(*(V[:, xs[:, i]] for i in range(4)))
    D = _tent(*(R[ys[:, j]] for j in range(4)))
    assert D.dtype == V.dtype
    return D


def up(V, W, H):
    """step 3's up(V) at the finer level's size W x H"""
    Hc, Wc = V.shape[:2]
    x, y = np.arange(W), np.arange(H)
    cx, cy = x >> 1, y >> 1
    nx, ny = np.clip(cx + np.where(x & 1, 1, -1), 0, Wc - 1), np.clip(cy + np.where(y & 1, 1, -1), 0, Hc - 1)
    at = lambda yy, xx: V[yy][:, xx]
    out = (U4[0] * at(cy, cx) + U4[1] * at(cy, nx)) + (U4[2] * at(ny, cx) + U4[3] * at(ny, nx))
    assert out.dtype == V.dtype
    return out


def glare_of(B, W, H, r):
    """steps 2-3 of B (n, 3): G, (H, W, 3)"""
    L, spread = int(r["levels"]), f32(r["spread"])
    D = [B.reshape(H, W, 3)]
    for _ in range(L):
        D.append(down(D[-1]))
    assert [(d.shape[1], d.shape[0]) for d in D] == sizes(W, H, L)
    U = D[L]
    for k in range(L - 1, 0, -1):
        U = D[k] + spread * up(U, D[k].shape[1], D[k].shape[0])
    G = up(U, W, H) * norm(spread, L)
    assert G.dtype == f32
    return G


def glare(c, A, W, H, r, e):
    return glare_of(bright(clean(c, A), threshold(r["threshold"], e)), W, H, r)


def bloom(c, A, W, H, r, e):
    """pt_bloom: (H, W, 4) float32"""
    G = glare(c, A, W, H, r, e).reshape(-1, 3)
    with np.errstate(all="ignore"):
        rgb = c + f32(r["intensity"]) * G
    assert rgb.dtype == f32
    return np.concatenate([rgb, A[:, None]], 1).reshape(H, W, 4)


def tonemap_bloom(c, A, tm_rule, r, T, W, H, prev=0.0):
    """(bytes, exposure, histogram) of pt_tonemap_bloom"""
    hist = TM.histogram(c, A)
    e = TM.exposure(hist, tm_rule, prev)
    out = bloom(c, A, W, H, r, e).reshape(-1, 4)
    return TM.apply(out[:, :3].copy(), out[:, 3].copy(), e, tm_rule, T, W, H), e, hist
