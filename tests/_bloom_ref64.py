"""include/pt_bloom.h's rule in float64, written apart from tests/_bloom_model.py (loops over taps on padded index arrays, not its gathers), and a
bound on |float32 result - this| that is derived, not fitted.

The inputs are the binary32 values the rule starts from: c and A (for FRAME, after the three divisions), T = threshold / exposure as the
binary32 quotient, spread and intensity.  norm is the exact 1 / (1 + spread + ... + spread^(L-1)) here; its binary32 roundings are counted below.

The bound.  u = 2^-24.  Every quantity of steps 0-3 is >= 0 and every weight is > 0, so a sum's rounding errors never cancel against the sum.
  Bright pass.  l = (a + b) + c of three rounded products: relative error <= 3u.  l - T: absolute error <= 3u*l + u*(l - T).  k = (l - T) / l:
    absolute error <= (3u*l + u*(l - T)) / l + 3u*k + u*k <= 8u, since k <= 1.  Where the two precisions disagree on l > T, |l - T| <= 3u*l and
    the k that is not 0 is <= 3u: inside the same 8u.  B = s * k: absolute error <= 8u*s + u*B <= 9u*s.  (Absolute in s, not relative in B: just
    above the threshold B is a small difference of large numbers.)
  The pyramid is linear in B with positive weights, so those errors arrive at G as at most 9u * P(s), P = steps 2-3 applied to s itself.
  Roundings along the longest path of a contribution to G: a tent is a product, an add and an add = 3, a level down two tents = 6, L levels = 6L;
    a level up is up()'s 3, the product with spread and the add to D_k = 5, L - 1 levels = 5(L - 1); the last up() 3 and the product with norm 1;
    norm itself L - 1 products and L - 1 adds, chained, and one division = 2(L - 1) + 1.  Together 13L - 2 < 13L: relative error
    <= (1 + u)^(13L) - 1 <= 1.01 * 13L * u  (13L <= 104, so the second order is far inside the 1 %).
  So |G32 - G64| <= E_G = 1.01*u * (13L * G64 + 9 * P(s)).
  Compose.  i * G: one rounding; c + that: one rounding of the result.  |out32 - out64| <= i * E_G + 1.01*u * (i*G64 + |c + i*G64|) + tiny, where
    tiny = 2^-126 covers the roundings of denormal intermediates (each at most 2^-150, a few hundred of them weighted by <= 1).
A pixel whose c is not finite has no bound (its output is that value, or NaN, in both)."""
import numpy as np

U = 2.0 ** -24


def _pad(n, m):
    """for the m outputs of a level reduced from n: the four tap indices, (4, m)"""
    return np.array([np.clip(2 * np.arange(m) - 1 + i, 0, n - 1) for i in range(4)])


def _down(V):
    H, W = V.shape[:2]
    Wd, Hd = (W + 1) // 2, (H + 1) // 2
    w = (0.125, 0.375, 0.375, 0.125)
    xs, ys = _pad(W, Wd), _pad(H, Hd)
    D = np.zeros((Hd, Wd, 3))
    for j in range(4):
        for i in range(4):
            D += w[i] * w[j] * V[ys[j]][:, xs[i]]
    return D


def _up(V, W, H):
    Hc, Wc = V.shape[:2]
    out = np.zeros((H, W, 3))
    for y in range(H):
        cy = y // 2
        ny = min(max(cy + (1 if y % 2 else -1), 0), Hc - 1)
        x = np.arange(W)
        cx = x // 2
        nx = np.clip(cx + np.where(x % 2 == 1, 1, -1), 0, Wc - 1)
        out[y] = 0.5625 * V[cy, cx] + 0.1875 * V[cy, nx] + 0.1875 * V[ny, cx] + 0.0625 * V[ny, nx]
    return out


def _pyramid(B, W, H, L, spread):
    D = [B.reshape(H, W, 3)]
    for _ in range(L):
        D.append(_down(D[-1]))
    Uk = D[L]
    for k in range(L - 1, 0, -1):
        Uk = D[k] + spread * _up(Uk, D[k].shape[1], D[k].shape[0])
    return _up(Uk, W, H) / sum(spread ** k for k in range(L))


def bloom(c, A, W, H, r, T):
    """(out (H, W, 4), bound (H, W, 3)) for the binary32 (c, A), the rule dict r and T = the binary32 threshold / exposure"""
    c64, A64 = np.asarray(c, np.float64), np.asarray(A, np.float64)
    L, spread, inten = int(r["levels"]), float(np.float32(r["spread"])), float(np.float32(r["intensity"]))
    with np.errstate(all="ignore"):
        s = np.where(np.isnan(c64), 0.0, np.clip(c64, 0.0, 65504.0))
        s = np.where((A64 > 0)[:, None], s, 0.0)
        wr, wg, wb = (float(np.float32(v)) for v in (0.2126, 0.7152, 0.0722))      # the rule's weights are the binary32 constants
        l = wr * s[:, 0] + wg * s[:, 1] + wb * s[:, 2]
        Tf = float(np.float32(T))
        k = np.where(l > Tf, (l - Tf) / np.where(l > 0, l, 1.0), 0.0)
    G =_pyramid(s * k[:, None], W, H, L, spread)
    P = _pyramid(s, W, H, L, spread)
    with np.errstate(all="ignore"):
        rgb = c64.reshape(H, W, 3) + inten * G
        EG = 1.01 * U * (13 * L * G + 9 * P)
        bound = inten * EG + 1.01 * U * (inten * G + np.abs(rgb)) + 2.0 ** -126
    return np.concatenate([rgb, A64.reshape(H, W, 1)], 2), bound
