"""A float64 evaluation of the a-trous denoiser as include/pt_denoise.h states it, with an exact exp, and the error bound a float32
implementation is held to against it (not a test module: the helpers of tests/test_denoise_ref.py and tests/test_gpu_denoise_ref.py).

Written from the header's text alone: every tap is a shifted rectangle of the image (a tap that would fall outside the image does not
exist), and the terms are divided as the formula writes them, sigma^2 * 4^-i included.

Error bound.  A float32 pass differs from this one through (a) the weights: the exponent e is a sum of a few rounded products (relative
error <= ~10u, u = 2^-24) and __expf adds ~2u relative plus e*u from scaling its argument, so a weight h*exp(-e) is off by at most
h*exp(-e)*(11e + 2)u <= h*(11/e_ + 2)u ~ 6.1u*h (the maximum of e*exp(-e) is 1/e_); summed over the taps that is <= 6.1u, and divided by
the centre weight (6/16)^2 that every valid pixel keeps, the weighted mean moves by at most 43u times the colour range R of its taps;
(b) the sums of w*c and w over 25 taps and the division: <= 51u times the largest colour magnitude M of the taps.  K passes add their
errors, and the mean FRAME.rgb / FRAME.a rounds once more, so a float32 result must lie within
    tol = u * (64*K*R + (64*K + 1)*M)
of this one, R and M taken over every pixel the K passes reach (the support).  The constants are 43 and 51 rounded up to 64."""
import numpy as np

U = 2.0 ** -24
H5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0


def classify(frame, feat):
    """(c, cls) in float64: the filter's input (mean FRAME.rgb / FRAME.a, raw rgb where FRAME.a <= 0) and 0 invalid, 1 hit, 2 miss"""
    fr = np.asarray(frame, np.float32).astype(np.float64)
    feat = np.asarray(feat, np.float32)
    a = fr[..., 3]
    with np.errstate(all="ignore"):
        mean = fr[..., :3] / a[..., None]
    g = feat[..., 0:7].astype(np.float64)
    valid = (a > 0) & np.isfinite(mean).all(-1) & np.isfinite(g).all(-1)
    miss = np.ascontiguousarray(feat[..., 7]).view(np.int32) == -1
    cls = np.where(valid, np.where(miss, 2, 1), 0)
    c = np.where((a > 0)[..., None], mean, fr[..., :3])
    return c, cls


def denoise(frame, feat, iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo):
    """(out, R, M): out = (H, W, 4) float64, rgb the denoised mean and a = FRAME.a; R, M = (H, W) colour range and largest colour magnitude
    over each pixel's support (see tol)"""
    frame = np.asarray(frame, np.float32)
    feat = np.asarray(feat, np.float32)
    H, W = frame.shape[:2]
    c, cls = classify(frame, feat)
    t = feat[..., 0].astype(np.float64)
    N = feat[..., 1:4].astype(np.float64)
    Kd = feat[..., 4:7].astype(np.float64)
    sn2, sd2, sa2 = float(sigma_normal) ** 2, float(sigma_depth) ** 2, float(sigma_albedo) ** 2
    lo, hi = c.copy(), c.copy()
    on = cls != 0
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            sc2 = float(sigma_color) ** 2 * 4.0 ** -i
            num = np.zeros((H, W, 3))
            den = np.zeros((H, W))
            nlo, nhi = lo.copy(), hi.copy()
            for dy in range(-2, 3):
                y0, y1 = max(0, -dy * s), min(H, H - dy * s)
                if y0 >= y1:
                    continue
                for dx in range(-2, 3):
                    x0, x1 = max(0, -dx * s), min(W, W - dx * s)
                    if x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))
                    same = (cls[P] != 0) & (cls[Q] == cls[P])
                    e = ((c[P] - c[Q]) ** 2).sum(-1) / sc2
                    dt = (t[P] - t[Q]) / t[P]
                    g = ((N[P] - N[Q]) ** 2).sum(-1) / sn2 + dt * dt / sd2 + ((Kd[P] - Kd[Q]) ** 2).sum(-1) / sa2
                    e = np.where(cls[P] == 1, e + g, e)
                    w = np.where(same, H5[dy + 2] * H5[dx + 2] * np.exp(-np.where(same, e, 0.0)), 0.0)
                    num[P] += w[..., None] * np.where(same[..., None], c[Q], 0.0)
                    den[P] += w
                    nlo[P] = np.where(same[..., None], np.minimum(nlo[P], lo[Q]), nlo[P])
                    nhi[P] = np.where(same[..., None], np.maximum(nhi[P], hi[Q]), nhi[P])
            c = np.where(on[..., None], num / den[..., None], c)
            lo, hi = nlo, nhi
        R = np.fmax.reduce(hi - lo, axis=-1)                 # fmax: the NaN channel of an invalid pixel does not hide the others
        M = np.fmax.reduce(np.fmax(np.abs(lo), np.abs(hi)), axis=-1)
    out = np.concatenate([c, frame[..., 3:4].astype(np.float64)], -1)
    return out, R, M


def tol(R, M, iterations):
    """the per-pixel bound of the module docstring"""
    K = int(iterations)
    return U * (64.0 * K * R + (64.0 * K + 1.0) * M)


def deviation(got, ref, R, M, iterations):
    """(worst, where): worst = the largest |got - ref| / tol over the finite pixels (<= 1 passes), and inf when a non-finite value of one
    side is not the same non-finite value on the other or the alpha differs; where = the (y, x) of it"""
    got = np.asarray(got, np.float64)
    nf = ~np.isfinite(ref[..., :3]) | ~np.isfinite(got[..., :3])
    same_nf = (got[..., :3] == ref[..., :3]) | (np.isnan(got[..., :3]) & np.isnan(ref[..., :3]))
    if (nf & ~same_nf).any():
        return float("inf"), tuple(int(v) for v in np.argwhere((nf & ~same_nf).any(-1))[0])
    if not np.array_equal(got[..., 3], ref[..., 3]):
        return float("inf"), tuple(int(v) for v in np.argwhere(got[..., 3] != ref[..., 3])[0])
    with np.errstate(all="ignore"):
        d = np.where(nf, 0.0, np.abs(got[..., :3] - ref[..., :3])).max(-1)
        bound = tol(R, M, iterations)
        r = np.where(d == 0, 0.0, d / bound)
    r = np.where(np.isnan(r), np.inf, r)
    k = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[k]), tuple(int(v) for v in k)
