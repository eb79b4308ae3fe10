"""The closest hit of a ray in a scene, by brute force in float64: every triangle of binding 3 and every ellipsoid of binding 7 is tested and the
minimum taken (not a test module: the helper of tests/test_intersect_ref64.py and tests/test_gpu_intersect_ref64.py).

This module knows no tree.  It reads bindings 3 and 7 and nothing else, and imports neither the oracle nor any model, so a box that is too small
anywhere between the builder and the intersect kernels — which both sides of every traversal-against-traversal comparison skip alike — shows
here as another hit.

The rule (rayScene, rayTri and rayEllipsoid of the shader), stated once more in float64:
  origin     o' = o + 1e-4 d
  triangle   e1 = v2 - v1, e2 = v3 - v1, p = d x e2, det = e1 . p, s = o' - v1, q = s x e1,
             u = (s . p) / det, v = (d . q) / det, t = (e2 . q) / det;
             a hit when |det| >= 1e-10, 0 <= u <= 1, v >= 0, u + v <= 1, t > 1e-10 (and t < 1e30); the smallest t wins, the lowest id among equals
  ellipsoid  oc = o' - c, a = f dx^2 + g dy^2 + h dz^2, b = 2 (f ocx dx + ...), C = f ocx^2 + ... - r^2, Disc = b^2 - 4 a C,
             t = (sqrt(Disc) - b) / 2a, tAlt = (-b - sqrt(Disc)) / 2a; a candidate when (Disc > 0 and tAlt > 0) or t > 0, with the value
             tAlt if t > tAlt else t — from inside that is the NEGATIVE near root; a square root of a negative Disc is a NaN and
             no comparison with it holds.  A rotated ellipsoid (|rot| > 0) sees o' and d each multiplied, as a row vector, by
             RX RY RZ (RZ = 1 when rot.z == 0) of the shader's rotationMatrix, with its centre left where it is.
  order      the ellipsoids follow the triangles, in index order, and each wins only with a value STRICTLY below the best so far.
The triangle products are evaluated as matrix products over (rays, triangles), through the identities (n = e1 x e2, w = o' x d)
  det = -d . n,   u det = w . e2 - d . (e2 x v1),   v det = -w . e1 - d . (v1 x e1),   t det = o' . n - v1 . n,
which are the triple products above with s = o' - v1 multiplied out; moller_trumbore() is the textbook form for one ray and one triangle, and
tests/test_intersect_ref64.py holds the two to each other.

Margins.  A float32 evaluation of the same rule may decide otherwise than this module wherever a comparison of the rule is close: that is the
contract's own behaviour (the kernels copy the shader's float32 arithmetic), and nothing this reference can judge.  Hit.robust() names the rays
on which no comparison is close; every margin is computed here, in float64, from the geometry alone:
  edge   over every triangle whose plane the ray meets in front (t > 0) and not beyond the winner's t (1 + 1e-4) — every such triangle when
         nothing wins —: the smallest distance of u and of v from 0 and from 1 and of u + v from 0 and from 1, less what float32 itself
         loses there: p = d x e2 and s . p round by a few 2^-24 |s| |d| |e2|, det by as much of |e1| |d| |e2|, so u (and v alike) is good to
         about UV_ROUND |d| e (|o'| + |v1| + e) / |det|, e the longer edge, |o'| + |v1| >= |s| (o' and v1 round too).     robust: > 1e-4
         (A grazed triangle makes this term large: with a flat 1e-4 the oracle and this module disagreed on rays 1.1e-4 to 8e-4 from an edge.)
  gap    (runner-up - winner) / |winner| over the accepted triangles and the ellipsoid candidates together.               robust: > 1e-4
  det    over the same triangles as `edge`, as far as they are not decisively outside (min(u, v, 1 - u - v) > -1e-4):
         (|det| - 1e-10) / (|e1| |e2| |d|); a float32 det carries a rounding error of a few 2^-24 of that product.          robust: > 2^-20
  front  over every triangle not decisively outside, in front or behind: |t - 1e-10| / (|o'|_inf + extent); a float32 t carries a few 2^-24
         of that length (more on a grazing ray, which `det` flags first).                                                 robust: > 2^-20
  ellip  over every ellipsoid: |Disc| / (b^2 + |4 a C|) and, where Disc > 0, |t| and |tAlt| over (|b| + sqrt(Disc)) / 2a.  robust: > 1e-4
`extent` is the largest absolute coordinate of any vertex or ellipsoid surface of the scene.

Work is done in chunks of rays so that the (rays, triangles) arrays stay below about 200 MB."""
import numpy as np

f64 = np.float64
PRIM_NONE = -1
PRIM_ELLIPSOID = 0x40000000
EPS = 1e-10
FAR = 1e30
EDGE, GAP, ROUND, ELLIP = 1e-4, 1e-4, 2.0 ** -20, 1e-4
UV_ROUND = 4.0 * 2.0 ** -24
WINDOW = 1.0 + 1e-4
_LIVE = 14                  # (rays, triangles) float64 arrays alive at once, at most
_BYTES = 200e6


class Hit:
    """per ray: t, u, v (float64; u = v = 0 unless a triangle wins), prim (int32: triangle id, PRIM_ELLIPSOID | i, PRIM_NONE), the margins of the
    module text, cos = |n . d| / |d| at the winner (n the unit normal of the winning surface; 1 with no winner), and `extent`"""

    def __init__(self, n, extent):
        self.t = np.full(n, FAR); self.u = np.zeros(n); self.v = np.zeros(n); self.prim = np.full(n, PRIM_NONE, np.int32)
        self.edge = np.full(n, np.inf); self.gap = np.full(n, np.inf); self.det = np.full(n, np.inf); self.front = np.full(n, np.inf)
        self.ellip = np.full(n, np.inf); self.cos = np.ones(n); self.extent = float(extent)
        self.slivers = 0        # triangles with two non-zero edges and no area to speak of (|e1 x e2| <= 2^-20 |e1| |e2|): float32 may hit them anywhere; the tests' scenes have none

    def robust(self):
        return (self.edge > EDGE) & (self.gap > GAP) & (self.det > ROUND) & (self.front > ROUND) & (self.ellip > ELLIP)

    def hit(self):
        return self.prim != PRIM_NONE


def moller_trumbore(o, d, v1, v2, v3):
    """the textbook form for one ray (o is o' already) and one triangle: (det, u, v, t)"""
    o, d, v1, v2, v3 = (np.asarray(x, f64) for x in (o, d, v1, v2, v3))
    e1, e2 = v2 - v1, v3 - v1
    p = np.cross(d, e2)
    det = e1 @ p
    s = o - v1
    q = np.cross(s, e1)
    with np.errstate(all="ignore"):
        return det, (s @ p) / det, (d @ q) / det, (e2 @ q) / det


def rotation_matrix(rot):
    """RX RY RZ of the shader's rotationMatrix, written row-major; a row vector is multiplied from the left: p' = p @ M"""
    x, y, z = (float(a) for a in rot)
    cx, sx, cy, sy = np.cos(x), np.sin(x), np.cos(y), np.sin(y)
    RX = np.array([[1, 0, 0], [0, cx, sx], [0, -sx, cx]], f64)
    RY = np.array([[cy, 0, -sy], [0, 1, 0], [sy, 0, cy]], f64)
    RZ = np.eye(3)
    if z != 0.0:
        cz, sz = np.cos(z), np.sin(z)
        RZ = np.array([[cz, sz, 0], [-sz, cz, 0], [0, 0, 1]], f64)
    return RX @ RY @ RZ


def ellipsoids(buffers):
    """binding 7 -> (c (n, 3), stretch (n, 3), rot (n, 3), r (n,)) in float64"""
    e = np.asarray(buffers[7], np.float32).astype(f64)
    n = int(e[0]) if e.size else 0
    return e[1:1 + 3 * n].reshape(n, 3), e[1 + 3 * n:1 + 6 * n].reshape(n, 3), e[1 + 6 * n:1 + 9 * n].reshape(n, 3), e[1 + 9 * n:1 + 10 * n]


def vertices(buffers):
    t = np.asarray(buffers[3], np.float32).astype(f64).reshape(-1, 40)
    return t[:, 0:3], t[:, 4:7], t[:, 8:11]


def scene_extent(buffers):
    v1, v2, v3 = vertices(buffers)
    c, st, _, r = ellipsoids(buffers)
    m = max([float(np.abs(v).max()) for v in (v1, v2, v3) if v.size] + [0.0])
    with np.errstate(all="ignore"):
        for i in range(len(r)):
            m = max(m, float((np.abs(c[i]) + np.abs(r[i]) / np.sqrt(np.abs(st[i]))).max()))      # the semi-axes are r / sqrt(f, g, h)
    return m


def _two_smallest(a):
    """(smallest, its column, second smallest) along axis 1 of a (c, m) array, m >= 1; the lowest column among equals"""
    k = np.argmin(a, axis=1)
    rows = np.arange(a.shape[0])
    best = a[rows, k]
    if a.shape[1] == 1:
        return best, k, np.full(a.shape[0], np.inf)
    keep = a[rows, k].copy()
    a[rows, k] = np.inf
    second = a.min(axis=1)
    a[rows, k] = keep
    return best, k, second


def _triangles(out, sl, o, d, tri):
    """the triangles' part for the rays of slice sl: fills t, u, v, prim, cos and the margins edge, det, front; -> the runner-up's t"""
    v1, e1, e2, n, e2xv1, v1xe1, v1n, scale, emax, v1len = tri
    w = np.cross(o, d)
    dn = np.linalg.norm(d, axis=1)
    length = np.abs(o).max(axis=1) + out.extent
    with np.errstate(all="ignore"):
        det = -(d @ n.T)
        inv = 1.0 / det
        u = (w @ e2.T - d @ e2xv1.T) * inv
        v = (-(w @ e1.T) - d @ v1xe1.T) * inv
        t = (o @ n.T - v1n[None, :]) * inv
        inside = np.minimum(np.minimum(u, v), 1.0 - u - v)                     # (u <= 1 follows from v >= 0 and u + v <= 1)
        ok = (np.abs(det) >= EPS) & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0) & (t > EPS) & (t < FAR)
        tt = np.where(ok, t, np.inf)
        best, k, second = _two_smallest(tt)
        rows = np.arange(o.shape[0])
        won = np.isfinite(best)
        out.t[sl] = np.where(won, best, FAR); out.prim[sl] = np.where(won, k, PRIM_NONE)
        out.u[sl] = np.where(won, u[rows, k], 0.0); out.v[sl] = np.where(won, v[rows, k], 0.0)
        out.cos[sl] = np.where(won, np.abs(det[rows, k]) / (np.linalg.norm(n[k], axis=1) * dn), 1.0)
        near = ~(inside <= -EDGE) & (scale > 0.0)[None, :]                    # not decisively outside; a triangle with a zero edge has det = 0 in every arithmetic
        out.front[sl] = np.where(near, np.abs(t - EPS) / length[:, None], np.inf).min(axis=1)
        return t, u, v, inside, near, det, second, scale, dn, emax, v1len, np.linalg.norm(o, axis=1)


def _window_margins(out, sl, parts, limit):
    """edge and det over the triangles in front and not beyond limit (per ray)"""
    t, u, v, inside, near, det, _, scale, dn, emax, v1len, reach = parts
    with np.errstate(all="ignore"):
        met = (t > 0.0) & (t <= limit[:, None]) & (scale > 0.0)[None, :]
        s = u + v
        dist = np.minimum.reduce([np.abs(u), np.abs(u - 1.0), np.abs(v), np.abs(v - 1.0), np.abs(s), np.abs(s - 1.0)])
        dist -= UV_ROUND * dn[:, None] * emax[None, :] * (reach[:, None] + v1len[None, :] + emax[None, :]) / np.abs(det)
        out.edge[sl] = np.where(met, dist, np.inf).min(axis=1)
        out.det[sl] = np.where(met & near, (np.abs(det) - EPS) / (scale[None, :] * dn[:, None]), np.inf).min(axis=1)


def _ellipsoids(out, sl, o, d, ell, second):
    """the ellipsoids' part, after the triangles: may replace t, prim, cos; fills ellip and gap"""
    c, st, rot, r = ell
    t_best, prim, cos = out.t[sl].copy(), out.prim[sl].copy(), out.cos[sl].copy()
    cands = [np.where(prim != PRIM_NONE, t_best, np.inf), second]
    margin = np.full(o.shape[0], np.inf)
    with np.errstate(all="ignore"):
        for i in range(len(r)):
            oo, dd = o, d
            if np.linalg.norm(rot[i]) > 0.0:
                M = rotation_matrix(rot[i])
                oo, dd = o @ M, d @ M
            f = st[i]
            oc = oo - c[i]
            a = (f * dd * dd).sum(axis=1)
            b = 2.0 * (f * oc * dd).sum(axis=1)
            C = (f * oc * oc).sum(axis=1) - r[i] * r[i]
            disc = b * b - 4.0 * a * C
            sq = np.sqrt(disc)
            t = (sq - b) / (2.0 * a)
            alt = (-b - sq) / (2.0 * a)
            cand = ((disc > 0.0) & (alt > 0.0)) | (t > 0.0)
            val = np.where(t > alt, alt, t)
            m = np.abs(disc) / (b * b + np.abs(4.0 * a * C))
            roots = np.minimum(np.abs(t), np.abs(alt)) / ((np.abs(b) + sq) / np.abs(2.0 * a))
            margin = np.minimum(margin, np.where(disc > 0.0, np.minimum(m, roots), m))
            cands.append(np.where(cand, val, np.inf))
            take = cand & (val < t_best)
            p = oo + val[:, None] * dd - c[i]                                  # the surface normal there, in the ellipsoid's frame
            g = f * p
            cs = np.abs((g * dd).sum(axis=1)) / (np.linalg.norm(g, axis=1) * np.linalg.norm(dd, axis=1))
            t_best = np.where(take, val, t_best); prim = np.where(take, PRIM_ELLIPSOID | i, prim); cos = np.where(take, cs, cos)
        tri_won = (prim & PRIM_ELLIPSOID) == 0
        out.u[sl] = np.where(tri_won, out.u[sl], 0.0); out.v[sl] = np.where(tri_won, out.v[sl], 0.0)
        out.t[sl], out.prim[sl], out.cos[sl], out.ellip[sl] = t_best, prim.astype(np.int32), cos, margin
        all_t = np.stack(cands, axis=1)
        best, _, runner = _two_smallest(all_t)
        out.gap[sl] = np.where(np.isfinite(best), (runner - best) / np.abs(best), np.inf)


def closest_hit(buffers, o, d):
    """o, d: (n, 3) rays as the kernels receive them (float32 values) -> Hit"""
    o32 = np.asarray(o, np.float32).reshape(-1, 3); d = np.asarray(d, np.float32).reshape(-1, 3).astype(f64)
    o = o32.astype(f64) + 1e-4 * d
    v1, v2, v3 = vertices(buffers)
    e1, e2 = v2 - v1, v3 - v1
    n = np.cross(e1, e2)
    l1, l2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
    tri = (v1, e1, e2, n, np.cross(e2, v1), np.cross(v1, e1), (v1 * n).sum(axis=1), l1 * l2, np.maximum(l1, l2), np.linalg.norm(v1, axis=1))
    ell = ellipsoids(buffers)
    out = Hit(o.shape[0], scene_extent(buffers))
    out.slivers = int(((tri[7] > 0.0) & (np.linalg.norm(n, axis=1) <= ROUND * tri[7])).sum())
    m = max(len(v1), 1)
    step = max(1, int(_BYTES / (8 * _LIVE * m)))
    for first in range(0, o.shape[0], step):
        sl = slice(first, min(first + step, o.shape[0]))
        second = np.full(sl.stop - sl.start, np.inf)
        parts = None
        if len(v1):
            parts = _triangles(out, sl, o[sl], d[sl], tri)
            second = parts[6]
        _ellipsoids(out, sl, o[sl], d[sl], ell, second)
        if parts is not None:                                                 # the window is the final winner's: a triangle behind an ellipsoid hit is not met
            limit = np.where(out.prim[sl] != PRIM_NONE, out.t[sl] * WINDOW, np.inf)
            _window_margins(out, sl, parts, limit)
    return out
