"""Which old pixel saw this surface point, and where between pixel centres: the reprojection calls' answer in float64, from the scene and the two
cameras alone (not a test module: the helper of tests/test_reproject_ref64.py and tests/test_gpu_reproject_ref64.py).

This module reads bindings 0, 1 and 4 of the image's camera A and of the current camera B, bindings 3, 7 and 14 of the current scene and, for the
moved calls, bindings 3 and 7 as they were at the mark.  It imports tests/_intersect_ref64.py (the brute-force closest hit) and nothing else: no
model, no feature record, no oracle.  A mistake that include/pt_reproject.h, its float32 twins and k_reproject share shows here as another pixel.

The camera.  camera_dirs() is main()'s lens-centre ray (frag.glsl:894-908) in float64: pixel (x, y) looks along q M, q = (-(2 tx - 1) ss,
(2 ty - 1) hr ss, fl), tx = (x + 0.5) / W, ty = (y + 0.5) / H, M = RX RY RZ.  project() is its inverse: q = X M^-1 (M^-1 by numpy, not by
transposition), scaled to q2 = fl, solved for tx and ty; (sx, sy) = (tx W, ty H) are in pixels with centres at the half-integers.

Per new pixel p.  B's ray through p's centre goes through closest_hit in the current scene.  A miss projects its direction.  A triangle hit k
with (u, v) is the point P = (1 - u - v) v1 + u v2 + v v3 on the current vertices, and P' is the same weights on the mark's vertices (no Gram
matrix).  An ellipsoid hit is P = o' + t d; on a moved one the point keeps its coordinates on the unit sphere, n_i = sqrt(f_i) (P_i - c_i) / r
from the surface equation sum f_i (x_i - c_i)^2 = r^2, so P'_i = c'_i + n_i r' / sqrt(f'_i); a moved ellipsoid with a rotation then or now is
rejected.  (sx, sy, q2) = project(P' - O') in A.  The old view is closest_hit along A's ray through every pixel centre, in the scene of the mark.
A primitive's material is float 36 of its binding-3 record or the last block of binding 7; a material is view-dependent as the header words it
(Pr != 1, Pc != 0, Tr > 0, Tf[0] > 0, illum 5 or 7, a map_Pr, map_Pc or map_Tr), read from binding 14.

Decision with normal_tol = -1 (material and depth alone decide).  For a new pixel and one old pixel s:
  must reject  behind A (q2 < 0); off the image by more than MARGIN_PX; s a miss against a hit or the reverse; another material;
               | |P' - O'| - t'_s | / t'_s above depth_tol by more than MARGIN_DEPTH; a view-dependent material without all_materials; a moved
               rotated ellipsoid
  must keep    on the image by more than MARGIN_PX, the same class and material, the depth ratio below depth_tol by more than MARGIN_DEPTH
  undecided    either primary hit is not Hit.robust(); sx or sy within MARGIN_PX of a whole number (nearest) or wx, wy within it of 0, snap,
               1 - snap, 1 (bilinear); the depth ratio within MARGIN_DEPTH of depth_tol; anything not finite.
Nearest: s = (floor(sy), floor(sx)).  Bilinear: each of the four taps gets the decision, a pixel is decided when all its taps of non-zero
weight are, and the expected result is the float64 weighted mean over the counting taps with the float64 weights after the snapping rule.

Margins.  MARGIN_PX = 2^-8 px: a float32 evaluation of steps 2-4 is off by a few 1e-4 px at these sizes (the bound of
tests/test_reproject_ref64.py measures it), and the kernels place P 1e-4 short of the surface along the ray (t is counted from o + 1e-4 d, the
header adds it to o), which is up to 1e-3 px under the dolly of the cases; 2^-8 clears both and costs under 2 % of the pixels per axis.
MARGIN_DEPTH = 1e-3: the same 1e-4 over a t' of 0.1 or more, and float32's rounding of |v| and t', a few 1e-7.

Probe images.  a(x, y) = 1 + (x + 3 y) mod 7; FRAME = ((x + 0.5) a, (y + 0.5) a, a, a), T = (a (x + 0.5), a (y + 0.5), a, 0).  A kept pixel's
rgb / a names its source's centre (nearest) or the centroid of its counting taps (bilinear) and a their weighted count; the four neighbours of
any point have four different counts, so a pins which taps counted."""
import numpy as np

import _intersect_ref64 as R64

f64 = np.float64
f32 = np.float32
MARGIN_PX = 2.0 ** -8
MARGIN_DEPTH = 1e-3
A_MAX = 7.0
TAPS = [(0, 0), (1, 0), (0, 1), (1, 1)]


# ---------------------------------------------------------------------------------------------------------------- the camera

class Camera:
    """bindings 0, 1, 4 of one view: O (and O32, the float32 words), M = RX RY RZ, ss, fl, hr"""

    def __init__(self, origin, rotation, params):
        self.O32 = np.ascontiguousarray(np.asarray(origin, f32)[:3])
        self.O = self.O32.astype(f64)
        ax, ay, az = np.asarray(rotation, f32)[:3].astype(f64)
        cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
        RX = np.array([[1, 0, 0], [0, cx, sx], [0, -sx, cx]])
        RY = np.array([[cy, 0, -sy], [0, 1, 0], [sy, 0, cy]])
        RZ = np.array([[cz, sz, 0], [-sz, cz, 0], [0, 0, 1]]) if az != 0 else np.eye(3)
        self.M = RX @ RY @ RZ
        P = np.asarray(params, f32).astype(f64)
        self.ss, self.fl, self.hr = P[0], P[1], P[3]

    @classmethod
    def of(cls, buffers):
        return cls(buffers[0], buffers[1], buffers[4])

    def dirs(self, W, H):
        """(H, W, 3): main() frag.glsl:894-908 with the lens offset zero: normalize(ORIGIN + direction * focus - ORIGIN)"""
        y, x = np.mgrid[0:H, 0:W]
        tcx, tcy = (x + 0.5) / W, (y + 0.5) / H
        q = np.stack([(tcx * 2 - 1) * -1 * self.ss, (tcy * 2 - 1) * self.hr * self.ss, np.full(x.shape, self.fl)], -1)
        d = q @ self.M
        return d / np.linalg.norm(d, axis=-1, keepdims=True)      # focus > 0 in every scene here: the focal distance only scales


def camera_dirs(wl, W, H):
    """the lens-centre ray of every pixel of a workload's camera, in float64"""
    return Camera.of(wl.buffers).dirs(W, H)


def project(X, cam, W, H):
    """(sx, sy, q2) of points relative to the camera (P - O), or of directions: the inverse of Camera.dirs.  q2 is the component along the
    camera's axis; sx and sy mean nothing unless q2 > 0."""
    q = np.asarray(X, f64) @ np.linalg.inv(cam.M)
    with np.errstate(all="ignore"):
        k = q[..., 2] / cam.fl                                     # q = k (-(2 tx - 1) ss, (2 ty - 1) hr ss, fl)
        tx = (1.0 - q[..., 0] / (k * cam.ss)) / 2.0
        ty = (1.0 + q[..., 1] / (k * cam.hr * cam.ss)) / 2.0
    return tx * W, ty * H, q[..., 2]


# ---------------------------------------------------------------------------------------------------------------- the scene

def view_dependent(mtl14):
    """bool per material of binding 14 (records of mtl[0] floats, the first at float 0)"""
    m = np.asarray(mtl14, f32).astype(f64)
    me = int(m[0])
    n = (m.size - 1) // me
    out = np.zeros(n, bool)
    for k in range(n):
        F = m[me * k: me * k + me]
        Pr, Pc, Tr, Tf0, illum = F[26], F[28], F[12], F[13], int(F[21])
        maps = [int(F[j]) for j in (33, 35, 39)]                   # map_Pr, map_Pc, map_Tr
        out[k] = Pr != 1 or Pc != 0 or Tr > 0 or Tf0 > 0 or illum in (5, 7) or any(j >= 0 for j in maps)
    return out


def materials(scene, prim):
    """the material of every primitive id of a Hit (-1 where nothing is hit)"""
    tri = np.asarray(scene[3], f32).reshape(-1, 40)[:, 36].astype(np.int64)
    e = np.asarray(scene[7], f32).ravel()
    ne = int(e[0]) if e.size else 0
    emat = e[1 + 10 * ne: 1 + 11 * ne].astype(np.int64)
    prim = np.asarray(prim, np.int64)
    hit = prim != R64.PRIM_NONE
    ell = hit & ((prim & R64.PRIM_ELLIPSOID) != 0)
    out = np.full(prim.shape, -1, np.int64)
    t = hit & ~ell
    out[t] = tri[prim[t]]
    out[ell] = emat[prim[ell] & 0xFFFFFF]
    return out


class View:
    """the closest hit of the lens-centre ray of every pixel of a camera in a scene ({3, 7}), flat over H * W"""

    def __init__(self, scene, cam, W, H):
        self.d = cam.dirs(W, H).astype(f32).reshape(-1, 3)
        self.o = np.broadcast_to(cam.O32, self.d.shape)
        self.hit = R64.closest_hit(scene, self.o, self.d)
        self.is_hit = self.hit.hit()
        self.robust = self.hit.robust()
        self.ell = self.is_hit & ((self.hit.prim & R64.PRIM_ELLIPSOID) != 0)
        self.mat = materials(scene, self.hit.prim)
        self.t = self.hit.t


def surface_points(scene_now, scene_then, view):
    """(P, P', forced): the surface point of every hit of `view` now, the same point at the mark, and the hits on a moved rotated ellipsoid"""
    n = view.d.shape[0]
    d = view.d.astype(f64)
    o = view.o.astype(f64) + 1e-4 * d
    P = o + view.t[:, None] * d
    Pp = P.copy()
    forced = np.zeros(n, bool)
    tri = view.is_hit & ~view.ell
    k = view.hit.prim[tri].astype(np.int64)
    u, v = view.hit.u[tri][:, None], view.hit.v[tri][:, None]
    for dst, sc in ((P, scene_now), (Pp, scene_then)):
        v1, v2, v3 = R64.vertices(sc)
        dst[tri] = (1.0 - u - v) * v1[k] + u * v2[k] + v * v3[k]
    c, st, rot, r = R64.ellipsoids(scene_now)
    c_, st_, rot_, r_ = R64.ellipsoids(scene_then)
    for i in range(len(r)):
        on = view.ell & ((view.hit.prim & 0xFFFFFF) == i)
        if not on.any():
            continue
        same = all(np.array_equal(a[i], b[i]) for a, b in ((c, c_), (st, st_), (rot, rot_), (r, r_)))
        if same:
            continue
        if np.any(rot[i] != 0) or np.any(rot_[i] != 0):
            forced |= on
            continue
        unit = np.sqrt(st[i]) * (P[on] - c[i]) / r[i]
        Pp[on] = c_[i] + unit * r_[i] / np.sqrt(st_[i])
    return P, Pp, forced


# ---------------------------------------------------------------------------------------------------------------- the probe images

def probe_count(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return (1 + (x + 3 * y) % 7).astype(f64)


def probe_images(W, H):
    """(FRAME, T) float32 (H, W, 4): exact in binary32"""
    y, x = np.mgrid[0:H, 0:W]
    a = probe_count(W, H)
    fr = np.stack([(x + 0.5) * a, (y + 0.5) * a, a, a], -1).astype(f32)
    T = np.stack([a * (x + 0.5), a * (y + 0.5), a, np.zeros_like(a)], -1).astype(f32)
    return fr, T


# ---------------------------------------------------------------------------------------------------------------- the reference

class Expect:
    """per pixel (H, W): decided, kept, and on kept pixels mean_x, mean_y (pixels, centres at half-integers), count (before the cap), ws (the
    sum of the counting taps' weights), taps (how many count); src_x, src_y for the nearest rule"""


class Reference:
    """now, then: {3, 7} of the current scene and of the scene at the mark (the same dict for the static calls); mtl14: binding 14; cam_a, cam_b:
    Camera of the image and of the current inputs."""

    def __init__(self, now, then, mtl14, cam_a, cam_b, W, H, depth_tol=0.02, all_materials=False, views=None):
        self.W, self.H, self.depth_tol = W, H, float(depth_tol)
        self.new, self.old = views or (View(now, cam_b, W, H), View(then, cam_a, W, H))      # views: those of the same scenes and cameras, made before
        new = self.new
        self.P, self.Pp, forced = surface_points(now, then, new)
        X = np.where(new.is_hit[:, None], self.Pp - cam_a.O, new.d.astype(f64))
        self.sx, self.sy, self.q2 = project(X, cam_a, W, H)
        self.dist = np.linalg.norm(self.Pp - cam_a.O, axis=1)
        vd = view_dependent(mtl14)
        mat_vd = np.zeros(new.mat.shape, bool)
        mat_vd[new.is_hit] = vd[new.mat[new.is_hit]]
        self.forced = forced | (mat_vd & (not all_materials))
        self.behind = self.q2 < 0
        with np.errstate(all="ignore"):
            self.finite = np.isfinite(self.sx) & np.isfinite(self.sy) & np.isfinite(self.q2) & np.isfinite(self.dist)
            m = MARGIN_PX
            self.off = ~self.behind & ((self.sx < -m) | (self.sx > W + m) | (self.sy < -m) | (self.sy > H + m))
            self.on = ~self.behind & (self.sx > m) & (self.sx < W - m) & (self.sy > m) & (self.sy < H - m)
        # a pixel whose fate no old pixel can change
        self.rejected = new.robust & (self.forced | (self.finite & (self.behind | self.off)))
        # the length one unit of intersection's bound moves the projected point by, in pixels (tests/_intersect_cases.unit)
        t = np.where(new.is_hit, np.abs(new.t), 0.0)
        unit_t = 2.0 ** -24 * (np.abs(new.o.astype(f64)).max(axis=1) + t + new.hit.extent) / new.hit.cos
        with np.errstate(all="ignore"):
            scale = cam_a.fl / (2.0 * cam_a.ss * np.abs(self.q2))
            self.unit_x = unit_t * W * scale + 2.0 ** -24 * W
            self.unit_y = unit_t * H * scale / cam_a.hr + 2.0 ** -24 * H

    def _tap(self, tx, ty):
        """(decided, counts) of every new pixel against the old pixel (tx, ty): int arrays over H * W"""
        W, H, new, old = self.W, self.H, self.new, self.old
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        s = np.where(inside, ty * W + tx, 0)
        oh, ot, om, orob = old.is_hit[s], old.t[s], old.mat[s], old.robust[s]
        with np.errstate(all="ignore"):
            ratio = np.abs(self.dist - ot) / ot
        same = oh & (om == new.mat)
        far = ratio > self.depth_tol + MARGIN_DEPTH
        near = ratio < self.depth_tol - MARGIN_DEPTH
        keep_hit = inside & same & near
        drop_hit = ~inside | ~oh | (om != new.mat) | far
        keep = np.where(new.is_hit, keep_hit, inside & ~oh)
        drop = np.where(new.is_hit, drop_hit, ~inside | oh)
        decided = ~inside | (orob & (keep | drop))
        return decided, keep & decided

    def nearest(self):
        """Expect of pt_reproject_frame / pt_reproject_frame_moved"""
        W, H, n = self.W, self.H, self.W * self.H
        m = MARGIN_PX
        with np.errstate(all="ignore"):
            whole = (np.abs(self.sx - np.rint(self.sx)) <= m) | (np.abs(self.sy - np.rint(self.sy)) <= m)
            ok = self.new.robust & self.finite & ~self.forced & self.on & ~whole
            ix = np.where(ok, np.floor(self.sx), 0).astype(np.int64)
            iy = np.where(ok, np.floor(self.sy), 0).astype(np.int64)
        dec, cnt = self._tap(ix, iy)
        e = Expect()
        e.decided = (self.rejected | (ok & dec)).reshape(H, W)
        e.kept = (ok & dec & cnt).reshape(H, W)
        a = probe_count(W, H).ravel()
        e.src_x, e.src_y = ix.reshape(H, W), iy.reshape(H, W)
        e.mean_x, e.mean_y = (ix + 0.5).reshape(H, W), (iy + 0.5).reshape(H, W)
        e.count = a[np.clip(iy, 0, H - 1) * W + np.clip(ix, 0, W - 1)].reshape(H, W)
        e.ws = np.ones((H, W))
        e.taps = e.kept.astype(np.int64)
        e.blended = np.zeros((H, W), bool)
        e.unit_x, e.unit_y = self.unit_x.reshape(H, W), self.unit_y.reshape(H, W)
        return e

    def _axis(self, s, snap):
        """the first tap's coordinate, the second tap's weight after snapping, and whether the weight clears every threshold by the margin"""
        m = MARGIN_PX
        with np.errstate(all="ignore"):
            f = s - 0.5
            c0 = np.floor(f)
            w = f - c0
            clear = np.ones(s.shape, bool)
            for th in {0.0, float(snap), 1.0 - float(snap), 1.0}:
                clear &= np.abs(w - th) > m
            lo = w < snap
            hi = ~lo & (w > 1.0 - snap)
            c0 = np.where(hi, c0 + 1.0, c0)
            w = np.where(lo | hi, 0.0, w)
        return c0, w, clear

    def bilinear(self, snap):
        """Expect of pt_reproject_frame_bilinear / pt_reproject_frame_moved_bilinear"""
        W, H, n = self.W, self.H, self.W * self.H
        x0, wx, cx = self._axis(self.sx, snap)
        y0, wy, cy = self._axis(self.sy, snap)
        ok = self.new.robust & self.finite & ~self.forced & self.on & cx & cy
        ix = np.where(ok, x0, 0).astype(np.int64)
        iy = np.where(ok, y0, 0).astype(np.int64)
        wx, wy = np.where(ok, wx, 0.0), np.where(ok, wy, 0.0)
        a = probe_count(W, H).ravel()
        dec = np.ones(n, bool)
        ws, sa, smx, smy, taps = (np.zeros(n) for _ in range(5))
        for i, j in TAPS:
            w = (wx if i else 1.0 - wx) * (wy if j else 1.0 - wy)
            tx, ty = ix + i, iy + j
            d, c = self._tap(tx, ty)
            live = w > 0
            dec &= d | ~live
            c = c & live
            s = np.clip(ty, 0, H - 1) * W + np.clip(tx, 0, W - 1)
            ws += np.where(c, w, 0.0)
            sa += np.where(c, w * a[s], 0.0)
            smx += np.where(c, w * (tx + 0.5), 0.0)
            smy += np.where(c, w * (ty + 0.5), 0.0)
            taps += c
        e = Expect()
        e.decided = (self.rejected | (ok & dec)).reshape(H, W)
        e.kept = (ok & dec & (taps > 0)).reshape(H, W)
        with np.errstate(all="ignore"):
            e.mean_x, e.mean_y, e.count = (smx / ws).reshape(H, W), (smy / ws).reshape(H, W), (sa / ws).reshape(H, W)
        e.ws = ws.reshape(H, W)
        e.taps = taps.astype(np.int64).reshape(H, W)
        e.blended = e.kept & (e.taps >= 2)
        e.src_x, e.src_y = ix.reshape(H, W), iy.reshape(H, W)
        e.unit_x, e.unit_y = self.unit_x.reshape(H, W), self.unit_y.reshape(H, W)
        return e


# ---------------------------------------------------------------------------------------------------------------- the comparison

class Found:
    """what compare() saw: n_decided, n_kept, wrong_decision and wrong_source (pixel counts), k (the largest multiple of the unit) and where"""

    def __init__(self):
        self.n_decided = self.n_kept = self.wrong_decision = self.wrong_source = 0
        self.k, self.where = 0.0, None

    def disagreements(self):
        return self.wrong_decision + self.wrong_source


def compare(e, frame, T, max_history):
    """An output FRAME (and T, or None) of a call on the probe images against an Expect.  A decided pixel must be kept or rejected as expected;
    a decided kept pixel must name the expected source: the old pixel its mean falls in (nearest: floor of the mean; bilinear: the centroid
    within half a pixel, and the count within half of the smallest difference between two taps' counts, 1, times the weight a tap can hide
    behind: |a - ref| < 0.5 / 1 when one tap counts).  k is the largest of |mean - ref| / unit and |a - ref| / (A_MAX unit) over the decided kept
    pixels, unit = (unit_x + unit_y) / ws: a tap weight is off by the error of sx plus that of sy, a centroid or a count is a ratio of sums
    of weights over ws, and a count is at most A_MAX."""
    frame = np.asarray(frame, f64)
    out = Found()
    kept = frame[..., 3] > 0
    d = e.decided
    out.n_decided, out.n_kept = int(d.sum()), int((d & e.kept).sum())
    out.wrong_decision = int((d & (kept != e.kept)).sum())
    sel = d & e.kept & kept
    if not sel.any():
        return out
    want_a = np.minimum(e.count, float(max_history))
    ks = []
    with np.errstate(all="ignore"):
        unit = (e.unit_x + e.unit_y) / e.ws
        images = [(frame[..., 0] / frame[..., 3], frame[..., 1] / frame[..., 3], frame[..., 3])]
        if T is not None:
            T = np.asarray(T, f64)
            images.append((T[..., 0] / T[..., 2], T[..., 1] / T[..., 2], T[..., 2]))
        wrong = np.zeros(d.shape, bool)
        for mx, my, a in images:
            dx, dy, da = np.abs(mx - e.mean_x), np.abs(my - e.mean_y), np.abs(a - want_a)
            one = e.taps == 1
            wrong |= sel & ~((dx < 0.5) & (dy < 0.5) & (da < 0.5))
            wrong |= sel & one & ((np.floor(mx) != np.floor(e.mean_x)) | (np.floor(my) != np.floor(e.mean_y)))
            ks.append(np.where(sel, np.maximum.reduce([dx / unit, dy / unit, da / (A_MAX * unit)]), 0.0))
    out.wrong_source = int(wrong.sum())
    k = np.maximum.reduce(ks)
    k = np.where(wrong, 0.0, np.nan_to_num(k, nan=np.inf))
    p = int(np.argmax(k))
    out.k, out.where = float(k.ravel()[p]), (p % e.decided.shape[1], p // e.decided.shape[1])
    return out
