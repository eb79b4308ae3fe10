"""float32 model of the reprojection across moved geometry of include/pt_motion.h, in the header's order (numpy float32 rounds every operation
as binary32, with no contraction), so that tests/test_gpu_motion.py can hold the device to it bit for bit.

Step 2's new part — the point P' where a hit's surface point was at the mark, and the normal N~ it had — is computed here; every other step is
tests/_reproject_model.py's (tests/_demod_model.py's step 7 with an albedo floor), reached by handing them records that make their own step 2
reproduce P': a hit's record gets t = 1, D = P' and N = N~ under a current origin of (-0, -0, -0), and (-0) + 1*x is x for every binary32 x, its
sign of zero included.  A hit the rule rejects gets t = NaN, which the shared step 2 rejects."""
import numpy as np

from _demod_model import reproject_demod
from _reproject_model import reproject

f32 = np.float32


def tri_vertices(buf3):
    """(n, 9) float32: A, B, C of every triangle of a binding-3 buffer (floats 0-2, 4-6, 8-10 of the 40-float records)"""
    t = np.asarray(buf3, f32).reshape(-1, 40)
    return np.ascontiguousarray(t[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]])


def ellipsoids(buf7):
    """(n, 10) float32: centre, stretch, rot, r of every ellipsoid of a binding-7 buffer ([count, centres, stretches, rots, radii, materials])"""
    e = np.asarray(buf7, f32).ravel()
    n = int(e[0]) if e.size else 0
    out = np.zeros((n, 10), f32)
    for i in range(n):
        out[i, 0:3] = e[1 + 3 * i: 4 + 3 * i]
        out[i, 3:6] = e[1 + 3 * n + 3 * i: 4 + 3 * n + 3 * i]
        out[i, 6:9] = e[1 + 6 * n + 3 * i: 4 + 6 * n + 3 * i]
        out[i, 9] = e[1 + 9 * n + i]
    return out


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def moved_point(rn, origin_n, tri_now, tri_then, el_now, el_then):
    """Step 2 for (n, 16) records: P' (n, 3), N~ (n, 3), rejected (n,) bool — the rejections this header adds — and kind (n,): 0 miss, 1 a hit on
    an unmoved primitive, 2 on a moved triangle, 3 on a moved ellipsoid (whether or not it is rejected)."""
    rn = np.ascontiguousarray(rn, f32).reshape(-1, 16)
    n = rn.shape[0]
    On = np.asarray(origin_n, f32)
    tri_now, tri_then = np.asarray(tri_now, f32).reshape(-1, 9), np.asarray(tri_then, f32).reshape(-1, 9)
    el_now, el_then = np.asarray(el_now, f32).reshape(-1, 10), np.asarray(el_then, f32).reshape(-1, 10)
    with np.errstate(all="ignore"):
        t, N, D = rn[:, 0], rn[:, 1:4], rn[:, 8:11]
        code = rn[:, 7].copy().view(np.int32)
        hit = code != -1
        P = On[None, :] + t[:, None] * D
        typ = code.view(np.uint32) >> 24
        k = (code & 0xffffff).astype(np.int64)
        Pp, Nt = P.copy(), N.copy()
        rej = np.zeros(n, bool)
        kind = np.where(hit, 1, 0)
        # triangles
        ntri = min(len(tri_now), len(tri_then))
        tri = hit & (typ == 1)
        rej |= tri & (k >= ntri)
        ti = np.nonzero(tri & (k < ntri))[0]
        if ti.size:
            now, then = tri_now[k[ti]], tri_then[k[ti]]
            mv = ~(now == then).all(1)
            ti, now, then = ti[mv], now[mv], then[mv]
        if ti.size:
            kind[ti] = 2
            A, B, C = now[:, 0:3], now[:, 3:6], now[:, 6:9]
            Ah, Bh, Ch = then[:, 0:3], then[:, 3:6], then[:, 6:9]
            e1, e2, w = B - A, C - A, P[ti] - A
            h1, h2 = Bh - Ah, Ch - Ah
            d11, d12, d22 = dot(e1, e1), dot(e1, e2), dot(e2, e2)
            den = d11 * d22 - d12 * d12
            w1, w2 = dot(w, e1), dot(w, e2)
            beta = (d22 * w1 - d12 * w2) / den
            gamma = (d11 * w2 - d12 * w1) / den
            pp = (Ah + beta[:, None] * h1) + gamma[:, None] * h2
            g, gh = cross(e1, e2), cross(h1, h2)
            Ni = N[ti]
            m1, m2 = dot(Ni, e1), dot(Ni, e2)
            a = (d22 * m1 - d12 * m2) / den
            b = (d11 * m2 - d12 * m1) / den
            c = dot(Ni, g) / dot(g, g)
            M = (a[:, None] * h1 + b[:, None] * h2) + c[:, None] * gh
            nt = M / np.sqrt(dot(M, M))[:, None]
            Pp[ti], Nt[ti] = pp, nt
            rej[ti] |= ~(np.isfinite(den) & (den > 0) & np.isfinite(pp).all(1) & np.isfinite(nt).all(1))
        # ellipsoids
        nel = min(len(el_now), len(el_then))
        el = hit & (typ == 3)
        rej |= el & (k >= nel)
        ei = np.nonzero(el & (k < nel))[0]
        if ei.size:
            now, then = el_now[k[ei]], el_then[k[ei]]
            mv = ~(now == then).all(1)
            ei, now, then = ei[mv], now[mv], then[mv]
        if ei.size:
            kind[ei] = 3
            rot = (now[:, 6:9] != 0).any(1) | (then[:, 6:9] != 0).any(1)
            u = P[ei] - now[:, 0:3]
            kk = np.sqrt(now[:, 3:6] / then[:, 3:6]) * (then[:, 9] / now[:, 9])[:, None]
            pp = then[:, 0:3] + u * kk
            Pp[ei] = pp
            rej[ei] |= rot | ~np.isfinite(pp).all(1)
        rej |= hit & (typ != 1) & (typ != 3)
    return Pp.astype(f32), Nt.astype(f32), rej, kind


def mapped_records(rn, fin_n, tri_now, tri_then, el_now, el_then):
    """the records and current inputs to hand to the shared steps (see the module's text)"""
    shape = np.asarray(rn).shape
    r = np.ascontiguousarray(rn, f32).reshape(-1, 16).copy()
    Pp, Nt, rej, _ = moved_point(r, fin_n["origin"], tri_now, tri_then, el_now, el_then)
    hit = r[:, 7].copy().view(np.int32) != -1
    bad = hit & (rej | ~np.isfinite(r[:, 0]) | ~np.isfinite(r[:, 1:4]).all(1) | ~np.isfinite(r[:, 8:11]).all(1))
    r[hit, 0] = f32(1)
    r[bad, 0] = f32(np.nan)
    r[hit, 1:4] = Nt[hit]
    r[hit, 8:11] = Pp[hit]
    # (an unmoved hit whose P overflowed fails the shared step 2's test of D here and step 4 on the device, where v is not finite: rejected either way)
    fin = dict(fin_n)
    fin["origin"] = np.array([-0.0, -0.0, -0.0], f32)
    return r.reshape(shape), fin


def reproject_moved(rn, rh, frame, T, fin_h, fin_n, mat_vd, rot_h, tri_now, tri_then, el_now, el_then, max_history, depth_tol, normal_tol,
                    all_materials=False, albedo_floor=0.0):
    """The new FRAME, the new T (None when T is None) and the kept count of pt_reproject_frame_moved.  rn: the records under the current inputs
    fin_n in the scene as it is now; rh: under the image's camera fin_h in the scene of the mark; tri_* / el_*: tri_vertices / ellipsoids of the
    two scenes' bindings 3 and 7; the rest as _reproject_model.reproject."""
    r, fin = mapped_records(rn, fin_n, tri_now, tri_then, el_now, el_then)
    if albedo_floor > 0:
        return reproject_demod(r, rh, frame, T, fin_h, fin, mat_vd, rot_h, max_history, depth_tol, normal_tol, all_materials, albedo_floor)
    return reproject(r, rh, frame, T, fin_h, fin, mat_vd, rot_h, max_history, depth_tol, normal_tol, all_materials)
