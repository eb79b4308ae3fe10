"""float32 model of the reprojection with bilinear taps of include/pt_reproject_bilinear.h, step by step in the header's order, on top of the models
of the calls it extends (tests/_reproject_model.py: the camera, the overlay; tests/_demod_model.py: the carried albedo).  numpy float32 rounds every
operation as binary32 with no contraction, so tests/test_gpu_reproject_bilinear.py can hold the device to it bit for bit (not a test module)."""
import numpy as np

from _demod_model import carried_albedo
from _guided_model import lum
from _reproject_model import overlay

f32 = np.float32
TAPS = [(0, 0), (1, 0), (0, 1), (1, 1)]                                   # (i, j): j outer, i inner


def project(rn, fin_h, fin_n, mat_vd, rot_h, W, H, all_materials=False):
    """Steps 2-4 of include/pt_reproject.h for (n, 16) records: ok, hit, v (n, 3), sx, sy"""
    n = rn.shape[0]
    M = np.asarray(rot_h, f32)
    Oh, On = fin_h["origin"], fin_n["origin"]
    ss, fl, hr = f32(fin_h["params"][0]), f32(fin_h["params"][1]), f32(fin_h["params"][3])
    mat_vd = np.asarray(mat_vd, np.uint8)
    t, N, D = rn[:, 0], rn[:, 1:4], rn[:, 8:11]
    code, mat = rn[:, 7].copy().view(np.int32), rn[:, 11].copy().view(np.int32)
    hit = code != -1                                                                              # 2
    matok = (mat >= 0) & (mat < mat_vd.size)
    vd = np.ones(n, bool)
    vd[matok] = mat_vd[mat[matok]] != 0
    ok = np.where(hit, np.isfinite(t) & np.isfinite(N).all(1) & np.isfinite(D).all(1) & matok & (bool(all_materials) | ~vd), True)
    P = On[None, :] + t[:, None] * D
    v = np.where(hit[:, None], P - Oh[None, :], D).astype(f32)
    v0, v1, v2 = v[:, 0], v[:, 1], v[:, 2]
    q = [(v0 * M[3 * i] + v1 * M[3 * i + 1]) + v2 * M[3 * i + 2] for i in range(3)]           # 3
    a = (q[0] / q[2]) * fl                                                                       # 4
    b = (q[1] / q[2]) * fl
    sx = ((f32(1) - a / ss) * f32(0.5)) * f32(W)
    sy = ((f32(1) + b / (hr * ss)) * f32(0.5)) * f32(H)
    ok = ok & (q[2] > 0) & (sx >= 0) & (sx < f32(W)) & (sy >= 0) & (sy < f32(H))
    return ok, hit, v, sx.astype(f32), sy.astype(f32)


def axis(s, snap):
    """step 5 along one axis: the first tap's coordinate (an int array) and the second tap's weight after snapping"""
    snap = f32(snap)
    f = (s - f32(0.5)).astype(f32)
    c0 = np.floor(f).astype(f32)
    w = (f - c0).astype(f32)
    lo = w < snap
    hi = ~lo & (w > f32(1) - snap)
    c0 = np.where(hi, c0 + f32(1), c0).astype(f32)
    w = np.where(lo | hi, f32(0), w).astype(f32)
    return c0.astype(np.int64), w


def reproject_bilinear(rn, rh, frame, T, fin_h, fin_n, mat_vd, rot_h, max_history, depth_tol, normal_tol, snap=1.0 / 64, all_materials=False, floor=0.0,
                       detail=False):
    """The new FRAME, the new T (None when T is None), the kept count and the blended count.  Arguments as _reproject_model.reproject; floor: the
    rule's albedo_floor.  detail: also a dict of the per-pixel count of counting taps (H, W) and the four taps' weights (4, H, W)."""
    H, W = frame.shape[:2]
    n = H * W
    rn = np.ascontiguousarray(rn, f32).reshape(n, 16)
    rh = np.ascontiguousarray(rh, f32).reshape(n, 16)
    fr = np.ascontiguousarray(frame, f32).reshape(n, 4)
    Tr = None if T is None else np.ascontiguousarray(T, f32).reshape(n, 4)
    mh = f32(max_history)
    demod = floor > 0
    with np.errstate(all="ignore"):
        ok, hit, v, sx, sy = project(rn, fin_h, fin_n, mat_vd, rot_h, W, H, all_materials)
        ok = ok & ~overlay(W, H, fin_n).ravel()                                                  # 1
        sx = np.where(ok, sx, f32(0.5)).astype(f32)
        sy = np.where(ok, sy, f32(0.5)).astype(f32)
        ix, wx = axis(sx, snap)                                                                  # 5
        iy, wy = axis(sy, snap)
        ax = [(f32(1) - wx).astype(f32), wx]
        ay = [(f32(1) - wy).astype(f32), wy]
        N, mat = rn[:, 1:4], rn[:, 11].copy().view(np.int32)
        ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        bn = carried_albedo(rn, floor) if demod else None
        cnt, src, wts = [], [], []
        for i, j in TAPS:
            tx, ty = ix + i, iy + j
            w = (ax[i] * ay[j]).astype(f32)
            inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            s = np.where(inside, ty * W + tx, 0)
            h = rh[s]
            ht, hN = h[:, 0], h[:, 1:4]
            hhit = h[:, 7].copy().view(np.int32) != -1
            hmat = h[:, 11].copy().view(np.int32)
            dot = (N[:, 0] * hN[:, 0] + N[:, 1] * hN[:, 1]) + N[:, 2] * hN[:, 2]
            hitok = hhit & (hmat == mat) & np.isfinite(ht) & (ht > 0) & (np.abs(ln - ht) <= f32(depth_tol) * ht) & (dot >= f32(normal_tol))
            F = fr[s]
            cnt.append(ok & (w > 0) & inside & np.where(hit, hitok, ~hhit) & (F[:, 3] > 0) & np.isfinite(F[:, :3]).all(1))
            src.append(s)
            wts.append(w)
        nc = sum(c.astype(np.int64) for c in cnt)
        out = np.zeros((n, 4), f32)                                                              # 6
        tout = None if Tr is None else np.zeros((n, 4), f32)

        # 7: exactly one counting tap s: step 7 of include/pt_reproject.h / include/pt_demod.h from s
        one = nc == 1
        s1 = np.zeros(n, np.int64)
        for c, s in zip(cnt, src):
            s1 = np.where(one & c, s, s1)
        F = fr[s1]
        o = F.copy()
        if demod:
            bh = carried_albedo(rh, floor)[s1]
            o[:, :3] = F[:, :3] * (bn / bh)
            rho = lum(bn) / lum(bh)
        cap = F[:, 3] > mh
        f = mh / F[:, 3]
        o[cap, :3] = o[cap, :3] * f[cap, None]
        o[cap, 3] = mh
        out[one] = o[one]
        if Tr is not None:
            Ts = Tr[s1]
            to = Ts.copy()
            if demod:
                to[:, 0] = Ts[:, 0] * rho
                to[:, 1] = (Ts[:, 1] * rho) * rho
            tcap = Ts[:, 2] > mh
            g = mh / Ts[:, 2]
            to[tcap, 0] = to[tcap, 0] * g[tcap]
            to[tcap, 1] = to[tcap, 1] * g[tcap]
            to[tcap, 2] = mh
            tout[one] = to[one]

        # 8, 9: two or more counting taps, accumulated from 0 in tap order
        many = nc >= 2
        zero = np.zeros(n, f32)
        Ws, A, C = zero.copy(), zero.copy(), np.zeros((n, 3), f32)
        WT, NT, Y, YY = zero.copy(), zero.copy(), zero.copy(), zero.copy()
        for c, s, w in zip(cnt, src, wts):
            F = fr[s]
            m = (F[:, :3] / F[:, 3:4]).astype(f32)
            if demod:
                bh = carried_albedo(rh, floor)[s]
                m = (m * (bn / bh)).astype(f32)
                rho = (lum(bn) / lum(bh)).astype(f32)
            Ws = np.where(c, Ws + w, Ws).astype(f32)
            A = np.where(c, A + w * F[:, 3], A).astype(f32)
            C = np.where(c[:, None], C + w[:, None] * m, C).astype(f32)
            if Tr is not None:
                Ts = Tr[s]
                ct = c & (Ts[:, 2] > 0) & np.isfinite(Ts[:, 0]) & np.isfinite(Ts[:, 1])
                y = (Ts[:, 0] / Ts[:, 2]).astype(f32)
                yy = (Ts[:, 1] / Ts[:, 2]).astype(f32)
                if demod:
                    y = (y * rho).astype(f32)
                    yy = ((yy * rho) * rho).astype(f32)
                WT = np.where(ct, WT + w, WT).astype(f32)
                NT = np.where(ct, NT + w * Ts[:, 2], NT).astype(f32)
                Y = np.where(ct, Y + w * y, Y).astype(f32)
                YY = np.where(ct, YY + w * yy, YY).astype(f32)
        mean = (C / Ws[:, None]).astype(f32)
        cn = (A / Ws).astype(f32)
        cn = np.where(cn > mh, mh, cn).astype(f32)
        o = np.concatenate([mean * cn[:, None], cn[:, None]], 1).astype(f32)
        out[many] = o[many]
        if Tr is not None:
            nT = (NT / WT).astype(f32)
            nT = np.where(nT > mh, mh, nT).astype(f32)
            to = np.stack([(Y / WT) * nT, (YY / WT) * nT, nT, zero], 1).astype(f32)
            sel = many & (WT > 0)
            tout[sel] = to[sel]
    kept, blended = int((nc >= 1).sum()), int(many.sum())
    res = (out.reshape(H, W, 4), None if tout is None else tout.reshape(H, W, 4), kept, blended)
    if detail:
        res += ({"taps": nc.reshape(H, W), "weights": np.stack(wts).reshape(4, H, W), "counts": np.stack(cnt).reshape(4, H, W),
                 "sx": sx.reshape(H, W), "sy": sy.reshape(H, W)},)
    return res
