"""A float64 evaluation of the variance-guided filter as include/pt_guided.h states it (and of its demodulated form, include/pt_demod.h), with an
exact exp, and the per-pixel error bound a float32 implementation is held to against it (not a test module: the helpers of
tests/test_guided_ref.py and tests/test_gpu_guided_ref.py).

Written from the two headers' text alone.  Every tap is a shifted rectangle of the image: a tap that would fall outside the image does not exist.

What stays float32.  The classification, the mean c = FRAME.rgb / FRAME.a, and the whole variance step (own s2, the pooled S, Q, N in row-major
tap order, max(x, 0) with NaN -> +inf, v = s2 / A), and for the demodulated form a_p, L_p, I_p = c_p / a_p and T', are evaluated here in float32
in the written order, exactly as the headers state them.  (Q - S*(S/N)) cancels, so how it rounds is part of the rule and not an error to bound;
the library is built without contraction, so the device rounds the same way, and these values are the common input of both sides: the bound starts
at zero.  From pass 0 on everything is float64: g_p, e_c, the edge terms as the formula divides them, exp, the sums, c' and v'.  The sigmas are the
float32 values the call receives, l()'s coefficients the float32 constants, 1e-10 and 1e-30 the decimal numbers.  A NaN follows IEEE: a hit with
t_p = 0 has (t_p - t_p) / t_p = NaN at its own tap, a NaN weight is not < 1e-30, so its c' and v' are NaN (deviation() asks for the same NaN).

Error bound, u = 2^-24, per pass and per pixel p, from this module's own float64 intermediates.  tol_q is the bound on |c - c_ref| of tap q
(largest channel) and av_q the bound on |v - v_ref| coming into the pass; both are 0 before pass 0.
  g_p      8 additions of non-negative terms (the k are powers of two) and a division, 9u relative, taken as 16u:
               dg = sum k av_q / sum k + 16u g.
  den      = sigma_lum*sqrt(g) + 1e-10: the root moves by at most sqrt(g + dg) - sqrt(max(g - dg, 0)); the root, the product, the sum, the
           constant's own rounding and a reciprocal or a division round 6 times, taken as 8u:
               dden = sigma_lum*(sqrt(g + dg) - sqrt(max(g - dg, 0))) + 8u den,  den_lo = max(den - dden, 1e-10 (1 - 8u)).
  l(c)     three products and two sums, each term rounded at most 3 times, taken as 4u, plus the incoming colour error (l's coefficients add to 1):
               dl_q = tol_q + 4u l(|c_q|).
  e_c      (a) the amplification: the colour error of the previous pass and the error of g_p enter through 1 / den,
               de_c = (dl_p + dl_q) / den_lo + e_c (dden / den_lo + 2u)        (the subtraction and the product round: 2u).
  edge     a difference, a square, a sum of three, the rounded 1/sigma^2 (2u) and a product: 8u; the depth term with its 1/t_p: 10u; the sum of
           the terms: 3u more; 13u, taken as 16u relative on the whole exponent, and 4u more for __expf scaling its argument by log2(e): 20u.
               de = de_c + 20u e;   e_lo = max(e - de, 0), e_hi = e + de.
  w        __expf is good to an ulp (2u) and h*exp rounds once (h(dx) h(dy) is exact): 3u, taken as 4u:
               w_hi = h exp(-e_lo) (1 + 4u),  w_lo = h exp(-e_hi) (1 - 4u).  The centre tap has e = 0 exactly and w = (6/16)^2 exactly on both sides.
  the cut  this module skips a tap when ITS w < 1e-30.  A tap whose [w_lo, w_hi] reaches 1e-30 (1 +- 2u) may fall on either side in float32: it is
           given to the bound, not to the result (w_lo = 0, and w_hi counts even where this module skipped it).  Such a weight is at most
           about 1e-30 against the centre's (6/16)^2 unless the pixel is ill-conditioned anyway, so the term is negligible; it is written down
           all the same.  dw_q = the largest |w - w_ref| these intervals allow.
  c'       with float32 weights w^ and colours c^: c^' - c' = sum w^ ((c_q - c') + (c^_q - c_q)) / sum w^, and sum w (c_q - c') = 0, so
               |c^' - c'| <= (sum dw_q |c_q - c'| + sum w_hi tol_q) / D_lo,  D_lo = sum w_lo >= (6/16)^2,
           with |c_q - c'| <= |c_q - c_p| + |c_p - c'|; and (b) 25 products and 24 sums in the numerator (25u of sum w |c_q|), 24 sums and a
           division below (25u of |c'|): 50u, taken as 64u of sum w |c_q| / sum w; products that underflow add 32 * 2^-149 / D_lo.
           A float32 c' is also a convex combination of its possible taps, so the bound never needs to exceed the distance from c' to the hull of
           [c_q - tol_q, c_q + tol_q] over them (plus the same rounding term): where the luminance term is ill-conditioned the bound saturates
           there and does not run away.
  v'       = sum w^2 v_q / (sum w)^2 by intervals, which to first order is twice the relative weight error plus the relative error of the
           incoming v: N_hi = sum w_hi^2 (v_q + av_q), N_lo = sum w_lo^2 max(v_q - av_q, 0), D_hi = sum w_hi;  w*w, *v and 24 sums round 27
           times, sw*sw and the division 50 times: 77u, taken as 128u:
               av' = max(N_hi / D_lo^2 (1 + 128u) - v', v' - N_lo / D_hi^2 (1 - 128u)) + 32 * 2^-149 (1 + max v_q) / D_lo^2   (w*w may underflow).
           v' = +inf is exact (av' = 0) unless the tap that makes it so, or its absence, hangs on a tap given to the bound: then av' = +inf.
The recursion is carried over each pixel's support as R and M are: tol and av of pass i are functions of those of its taps in pass i - 1.
Constants rounded up: 9 -> 16, 6 -> 8, 3 -> 4 (twice), 13 + 1 -> 20, 50 -> 64, 77 -> 128.
The demodulated output a_p * I_K rounds once more: bound a_p tol + u |a_p I_K| per channel.

A pixel is called UNINFORMATIVE when tol > 1e-3 R, R the colour range of its support, and tol also exceeds the summation term 64 K u M that no
conditioning affects (a support of one colour, R = 0, has nothing to inform about)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

STRIPS, STRIP_PIXELS = 8, 50000                                           # a large image is evaluated in 8 row strips, one thread each
U = 2.0 ** -24
ETA = 2.0 ** -149
INF = float("inf")
H5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
K3 = np.array([0.25, 0.5, 0.25])
f32 = np.float32
CUT = 1e-30


def lum32(c):
    c = np.asarray(c, f32)
    return (f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]) + f32(0.0722) * c[..., 2]


LC = np.array([float(f32(0.2126)), float(f32(0.7152)), float(f32(0.0722))])


def lum64(c):
    return (LC[0] * c[..., 0] + LC[1] * c[..., 1]) + LC[2] * c[..., 2]


def _rects(H, W, dy, dx, r0=0, r1=None):
    """the pixels p (of rows r0 .. r1 - 1) whose tap p + (dx, dy) is inside the image, and those taps: two index tuples, or None when there are none"""
    y0, y1 = max(r0, -dy), min(H if r1 is None else r1, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def _clamp_var32(x):
    return np.where(np.isnan(x), f32(np.inf), np.where(x >= 0, x, f32(0))).astype(f32)


def prepare(frame, feat, T, min_frames, floor=None):
    """The float32 part: a dict of cls (0 invalid, 1 hit, 2 miss), c (the filter's colour input: the mean, the illumination I on a valid hit of
    the demodulated form, the raw rgb where FRAME.a <= 0), v = s2 / A (0 on invalid pixels: never read), a and L (ones in the plain form)"""
    frame = np.asarray(frame, f32)
    feat = np.asarray(feat, f32)
    T = np.asarray(T, f32)
    H, W = frame.shape[:2]
    A = frame[..., 3]
    with np.errstate(all="ignore"):
        mean = (frame[..., :3] / A[..., None]).astype(f32)
        valid = (A > 0) & np.isfinite(mean).all(-1) & np.isfinite(feat[..., 0:7]).all(-1)
        miss = np.ascontiguousarray(feat[..., 7]).view(np.int32) == -1
        cls = np.where(valid, np.where(miss, 2, 1), 0)
        c = np.where((A > 0)[..., None], mean, frame[..., :3]).astype(f32)
        a = np.ones((H, W, 3), f32)
        L = np.ones((H, W), f32)
        sY, sYY, n = T[..., 0], T[..., 1], T[..., 2]
        if floor is not None:
            hit = cls == 1
            ap = np.fmax(feat[..., 4:7], f32(floor)).astype(f32)
            I = (c / ap).astype(f32)
            bad = hit & ~np.isfinite(I).all(-1)
            cls = np.where(bad, 0, cls)
            hit = cls == 1
            a = np.where(hit[..., None], ap, f32(1)).astype(f32)
            c = np.where(hit[..., None], I, c).astype(f32)
            L = np.where(hit, lum32(a), f32(1)).astype(f32)
            sY = np.where(hit, sY / L, sY).astype(f32)
            sYY = np.where(hit, (sYY / L) / L, sYY).astype(f32)
        mat = np.ascontiguousarray(feat[..., 11]).view(np.int32)
        m = (sY / n).astype(f32)
        own = _clamp_var32(((sYY - (sY * m).astype(f32)).astype(f32) / (n - f32(1)).astype(f32)).astype(f32))
        S = np.zeros((H, W), f32); Q = np.zeros((H, W), f32); N = np.zeros((H, W), f32)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                r = _rects(H, W, dy, dx)
                if r is None:
                    continue
                P, Qr = r
                use = (cls[P] != 0) & (cls[Qr] == cls[P]) & ((cls[P] != 1) | (mat[Qr] == mat[P])) & (n[Qr] >= f32(1))
                S[P] = np.where(use, (S[P] + sY[Qr]).astype(f32), S[P])
                Q[P] = np.where(use, (Q[P] + sYY[Qr]).astype(f32), Q[P])
                N[P] = np.where(use, (N[P] + n[Qr]).astype(f32), N[P])
        pooled = _clamp_var32(((Q - (S * (S / N).astype(f32)).astype(f32)).astype(f32) / (N - f32(1)).astype(f32)).astype(f32))
        pooled = np.where(N >= f32(2), pooled, f32(np.inf)).astype(f32)
        s2 = np.where(n >= f32(min_frames), own, pooled).astype(f32)
        v = np.where(cls != 0, (s2 / A).astype(f32), f32(0)).astype(f32)
    return {"cls": cls, "c": c, "v": v, "a": a, "L": L, "A": A}


def _pass(c, v, tol, av, lo, hi, cls, t, Nn, Kd, s, sl, sn2, sd2, sa2):
    """one pass of step s over (c, v) with the incoming bounds (tol, av) and support extremes (lo, hi): the same six after it"""
    H, W = cls.shape
    valid = cls != 0
    hitp = cls == 1
    # g_p and its error
    gs = np.zeros((H, W)); gk = np.zeros((H, W)); ga = np.zeros((H, W))
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            r = _rects(H, W, dy, dx)
            if r is None:
                continue
            P, Q = r
            use = valid[P] & (cls[Q] == cls[P])
            k = K3[dy + 1] * K3[dx + 1]
            gs[P] += np.where(use, k * v[Q], 0.0)
            ga[P] += np.where(use, k * av[Q], 0.0)
            gk[P] += np.where(use, k, 0.0)
    g = gs / gk
    dg = ga / gk + np.where(np.isinf(g), 0.0, 16 * U * g)
    lum_on = np.isfinite(sl) & ~np.isinf(g)
    lum_unsure = np.isfinite(sl) & np.isinf(dg)                          # whether g_p is +inf hangs on a tap given to the bound
    gf = np.where(lum_on, g, 0.0)
    dgf = np.where(lum_on & ~lum_unsure, dg, 0.0)
    slf = sl if np.isfinite(sl) else 0.0
    den = slf * np.sqrt(gf) + 1e-10
    dden = slf * (np.sqrt(gf + dgf) - np.sqrt(np.maximum(gf - dgf, 0.0))) + 8 * U * den
    den_lo = np.maximum(den - dden, 1e-10 * (1 - 8 * U))
    lc = lum64(c)
    dl = tol + 4 * U * lum64(np.abs(c))
    num = np.zeros((H, W, 3)); nab = np.zeros((H, W, 3)); sw = np.zeros((H, W))
    e1 = np.zeros((H, W, 3))                                              # sum dw |c_q - c_p|
    e2 = np.zeros((H, W)); e3 = np.zeros((H, W))                          # sum dw, sum w_hi tol_q
    d_lo = np.zeros((H, W)); d_hi = np.zeros((H, W))
    n_ref = np.zeros((H, W)); n_hi = np.zeros((H, W)); n_lo = np.zeros((H, W)); vmax = np.zeros((H, W))
    ref_inf = np.zeros((H, W), bool); sure_inf = np.zeros((H, W), bool); v_unsure = np.zeros((H, W), bool)
    t_lo = np.full((H, W, 3), INF); t_hi = np.full((H, W, 3), -INF)       # the hull of the possible taps
    nlo, nhi = lo.copy(), hi.copy()

    def strip(r0, r1):                                                    # rows r0 .. r1 - 1 of the pass: strips write disjoint rows
        with np.errstate(all="ignore"):                                   # (per thread)
            taps(r0, r1)

    def taps(r0, r1):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                r = _rects(H, W, dy * s, dx * s, r0, r1)
                if r is None:
                    continue
                P, Q = r
                same = valid[P] & (cls[Q] == cls[P])
                ec = np.where(lum_on[P], np.abs(lc[P] - lc[Q]) / den[P], 0.0)
                dec = np.where(lum_on[P], (dl[P] + dl[Q]) / den_lo[P] + ec * (dden[P] / den_lo[P] + 2 * U), 0.0)
                dec = np.where(lum_unsure[P], INF, dec)
                dt = (t[P] - t[Q]) / t[P]
                eg = dt * dt / sd2
                if np.isfinite(sn2):                                      # (a finite difference over +inf is 0: valid pixels have finite N and Kd)
                    eg = eg + ((Nn[P] - Nn[Q]) ** 2).sum(-1) / sn2
                if np.isfinite(sa2):
                    eg = eg + ((Kd[P] - Kd[Q]) ** 2).sum(-1) / sa2
                e = np.where(hitp[P], ec + eg, ec)
                w = H5[dy + 2] * H5[dx + 2] * np.exp(-e)
                de = dec + 20 * U * e
                if dy == 0 and dx == 0:
                    de = np.where(np.isnan(e), de, 0.0)
                big = np.isinf(e)
                w_hi = np.where(big, 0.0, H5[dy + 2] * H5[dx + 2] * np.exp(-np.where(big, 0.0, np.maximum(e - de, 0.0))) * (1 + 4 * U))
                w_lo = np.where(big, 0.0, H5[dy + 2] * H5[dx + 2] * np.exp(-np.where(big, 0.0, e + de)) * (1 - 4 * U))
                if dy == 0 and dx == 0:
                    w_hi = np.where(np.isnan(e), w_hi, w); w_lo = np.where(np.isnan(e), w_lo, w)
                inc = same & ~(w < CUT)                                       # the header's cut, on this module's own weight (a NaN stays in)
                maybe = same & ~(w_hi < CUT * (1 - 2 * U))                    # float32 may take the tap
                surely = same & ~(w_lo < CUT * (1 + 2 * U))                   # float32 takes the tap
                border = maybe & ~surely
                wr = np.where(inc, w, 0.0)
                whi = np.where(maybe, w_hi, 0.0)
                wlo = np.where(surely, w_lo, 0.0)
                dw = np.maximum(whi - wr, wr - wlo)
                cq = np.where(same[..., None], c[Q], 0.0)
                num[P] += wr[..., None] * np.where(inc[..., None], cq, 0.0)
                nab[P] += wr[..., None] * np.where(inc[..., None], np.abs(cq), 0.0)
                sw[P] += wr
                e1[P] += np.where(maybe[..., None], dw[..., None] * np.abs(cq - c[P]), 0.0)
                e2[P] += dw
                e3[P] += np.where(maybe, whi * tol[Q], 0.0)
                d_lo[P] += wlo
                d_hi[P] += whi
                vq, aq = v[Q], av[Q]
                qinf = np.isinf(vq)
                ref_inf[P] |= inc & qinf
                sure_inf[P] |= surely & inc & qinf & (aq == 0)
                v_unsure[P] |= (maybe & np.isinf(aq)) | (border & qinf)
                fin = maybe & ~qinf & ~np.isinf(aq)
                n_ref[P] += np.where(inc & ~qinf, wr * wr * np.where(qinf, 0.0, vq), 0.0)
                n_hi[P] += np.where(fin, whi * whi * (np.where(fin, vq, 0.0) + np.where(fin, aq, 0.0)), 0.0)
                n_lo[P] += np.where(fin, wlo * wlo * np.maximum(np.where(fin, vq, 0.0) - np.where(fin, aq, 0.0), 0.0), 0.0)
                vmax[P] = np.where(fin, np.maximum(vmax[P], vq), vmax[P])
                tq = tol[Q][..., None]
                t_lo[P] = np.where(maybe[..., None], np.minimum(t_lo[P], cq - tq), t_lo[P])
                t_hi[P] = np.where(maybe[..., None], np.maximum(t_hi[P], cq + tq), t_hi[P])
                nlo[P] = np.where(same[..., None], np.minimum(nlo[P], lo[Q]), nlo[P])
                nhi[P] = np.where(same[..., None], np.maximum(nhi[P], hi[Q]), nhi[P])

    if H * W >= STRIP_PIXELS and H >= 2 * STRIPS:
        edges = [H * k // STRIPS for k in range(STRIPS + 1)]
        with ThreadPoolExecutor(STRIPS) as ex:
            list(ex.map(lambda k: strip(edges[k], edges[k + 1]), range(STRIPS)))
    else:
        strip(0, H)
    c2 = num / sw[..., None]
    rnd = 64 * U * nab / sw[..., None] + 32 * ETA / d_lo[..., None]
    form = (e1 + e2[..., None] * np.abs(c - c2) + e3[..., None]) / d_lo[..., None] + rnd
    hull = np.maximum(t_hi - c2, c2 - t_lo) + rnd
    tol2 = np.fmin(form, hull)                                            # fmin: a NaN formula (inf * 0) leaves the hull
    tol2 = np.where(np.isnan(tol2), INF, tol2).max(-1)
    v2 = np.where(ref_inf, INF, n_ref / (sw * sw))
    up = n_hi / (d_lo * d_lo) * (1 + 128 * U) - v2
    dn = v2 - n_lo / (d_hi * d_hi) * (1 - 128 * U)
    av2 = np.maximum(np.maximum(up, dn), 0.0) + 32 * ETA * (1 + vmax) / (d_lo * d_lo)
    av2 = np.where(ref_inf, 0.0, av2)
    av2 = np.where(v_unsure & ~(ref_inf & sure_inf), INF, av2)
    av2 = np.where(np.isnan(av2), INF, av2)
    c_out = np.where(valid[..., None], c2, c)
    v_out = np.where(valid, v2, v)
    return c_out, v_out, np.where(valid, tol2, 0.0), np.where(valid, av2, 0.0), nlo, nhi


def filter64(frame, feat, T, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames, floor=None):
    """The reference.  A dict: out (H, W, 4) float64 (rgb = c_K, or a_p * I_K with a floor; a = FRAME.a), v (H, W) = v_K (of the illumination with
    a floor), bound_c (H, W, 3) and bound_v (H, W): what a float32 out and v_K may differ by; c (H, W, 3) = c_K or I_K, tol (H, W) its bound,
    R and M (H, W) the colour range and largest magnitude over each pixel's support, cls, a, L (prepare()'s), K.
    iterations may be a tuple of pass counts: then a dict of such dicts, one per count, from one run of the passes."""
    many = isinstance(iterations, (tuple, list))
    Ks = sorted(int(k) for k in iterations) if many else [int(iterations)]
    d = prepare(frame, feat, T, min_frames, floor)
    feat = np.asarray(feat, f32)
    alpha = np.asarray(frame, f32)[..., 3:4].astype(np.float64)
    cls = d["cls"]
    c = d["c"].astype(np.float64)
    v = d["v"].astype(np.float64)
    t = feat[..., 0].astype(np.float64)
    Nn = feat[..., 1:4].astype(np.float64)
    Kd = feat[..., 4:7].astype(np.float64)
    a = d["a"].astype(np.float64)
    sl, sn, sd, sa = (float(f32(x)) for x in (sigma_lum, sigma_normal, sigma_depth, sigma_albedo))
    tol = np.zeros(cls.shape); av = np.zeros(cls.shape)
    lo, hi = c.copy(), c.copy()
    res = {}
    with np.errstate(all="ignore"):
        for i in range(Ks[-1] + 1):
            if i in Ks:
                R = np.fmax.reduce(hi - lo, axis=-1)                      # fmax: the NaN channel of an invalid pixel does not hide the others
                M = np.fmax.reduce(np.fmax(np.abs(lo), np.abs(hi)), axis=-1)
                rgb = a * c if floor is not None else c
                bound_c = a * tol[..., None] + (U * np.abs(rgb) if floor is not None else 0.0)
                bound_c = np.where(np.isnan(bound_c), INF, bound_c)
                res[i] = {"out": np.concatenate([rgb, alpha], -1), "v": v, "bound_c": bound_c, "bound_v": av, "c": c, "tol": tol, "R": R, "M": M,
                          "cls": cls, "a": a, "L": d["L"].astype(np.float64), "K": i}
            if i < Ks[-1]:
                c, v, tol, av, lo, hi = _pass(c, v, tol, av, lo, hi, cls, t, Nn, Kd, 1 << i, sl, sn * sn, sd * sd, sa * sa)
    return res if many else res[Ks[0]]


def _worst(d, bound, bad):
    with np.errstate(all="ignore"):
        r = np.where(d == 0, 0.0, d / bound)
    r = np.where(np.isnan(r) | bad, np.inf, r)
    k = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[k]), tuple(int(x) for x in k[:2])


def deviation(got, ref):
    """(worst, where): the largest |got - ref.out| / ref.bound_c over the finite values (<= 1 passes; 0 / 0 counts as 0), and inf when a
    non-finite value of one side is not the same non-finite value on the other or the alpha differs; where = the (y, x) of it"""
    got = np.asarray(got, np.float64)
    want = ref["out"]
    g, w = got[..., :3], want[..., :3]
    nf = ~np.isfinite(g) | ~np.isfinite(w)
    same_nf = (g == w) | (np.isnan(g) & np.isnan(w))
    bad = (nf & ~same_nf) | (got[..., 3] != want[..., 3])[..., None]
    with np.errstate(all="ignore"):
        d = np.where(nf, 0.0, np.abs(g - w))
    return _worst(d, ref["bound_c"], bad)


def deviation_v(got_v, ref):
    """deviation() for a float32 v_K against ref.v within ref.bound_v, over the valid pixels"""
    g = np.asarray(got_v, np.float64)
    w = ref["v"]
    on = ref["cls"] != 0
    nf = on & (~np.isfinite(g) | ~np.isfinite(w))
    same_nf = (g == w) | (np.isnan(g) & np.isnan(w))
    with np.errstate(all="ignore"):
        d = np.where(nf | ~on, 0.0, np.abs(g - w))
    return _worst(d, ref["bound_v"], nf & ~same_nf & ~np.isinf(ref["bound_v"]))


def uninformative_share(ref):
    """the share of the valid pixels whose bound says nothing (see the module docstring)"""
    on = ref["cls"] != 0
    if not on.any():
        return 0.0
    with np.errstate(all="ignore"):
        un = on & ~((ref["tol"] <= 1e-3 * ref["R"]) | (ref["tol"] <= 64 * ref["K"] * U * ref["M"]))
    un &= ~np.isnan(ref["c"]).any(-1)                                     # a NaN result is compared as a NaN, not through the bound
    return float(un.sum()) / float(on.sum())


def select(ref, T, min_frames, rel_err, abs_err, max_frames, overlay=None, demod=False):
    """include/pt_steer.h's rule (include/pt_demod.h's step 5 when demod) on the reference's (c_K, v_K): (active, near, step).  Steps 1-4 are float32
    and exact.  near marks the step-5 pixels a float32 implementation may decide either way: |v_K L^2 - tol^2| within bound_v L^2 plus what bound_c
    moves tol^2 by, plus the few roundings of the two sides (4u each)."""
    T = np.asarray(T, f32)
    sY, sYY, n = T[..., 0], T[..., 1], T[..., 2]
    cls = ref["cls"]
    with np.errstate(all="ignore"):
        mean = (sY / n).astype(f32)
        var = ((sYY - (sY * mean).astype(f32)).astype(f32) / (n - f32(1)).astype(f32)).astype(f32)
        err2 = (var / n).astype(f32)
        tl = np.fmax((f32(rel_err) * np.abs(mean)).astype(f32), f32(abs_err)).astype(f32)
        own = err2 > (tl * tl).astype(f32)
        rgb = ref["out"][..., :3]
        tol = np.fmax(float(f32(rel_err)) * np.abs(lum64(rgb)), float(f32(abs_err)))
        dtol = float(f32(rel_err)) * lum64(ref["bound_c"]) + 8 * U * tol
        tol2 = tol * tol
        dtol2 = 2 * tol * dtol + dtol * dtol + 4 * U * tol2
        L2 = ref["L"] ** 2 if demod else 1.0
        vK = ref["v"] * L2
        dv = ref["bound_v"] * L2 + 4 * U * np.where(np.isfinite(vK), vK, 0.0)
        guided = np.isinf(ref["v"]) | (vK > tol2)
        near = ~np.isinf(ref["v"]) & ~(np.abs(vK - tol2) > dv + dtol2)     # a NaN on either side counts as near, not as decided
        near |= np.isinf(ref["bound_v"])
    act = np.where(cls == 0, own, guided)
    step = np.where(cls == 0, 4, 5)
    low = n < f32(min_frames)
    act = np.where(low, True, act)
    step = np.where(low, 3, step)
    if max_frames > 0:
        cap = n >= f32(max_frames)
        act = act & ~cap
        step = np.where(cap, 2, step)
    if overlay is not None:
        act = act & ~overlay
        step = np.where(overlay, 1, step)
    return act.astype(bool), near & (step == 5), step
