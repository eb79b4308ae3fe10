"""float32 model of include/pt_reproject_through.h: the rule step by step, in the header's order (numpy float32 rounds every operation as binary32,
with no contraction), so that tests/test_gpu_reproject_through.py can hold the device to it bit for bit.  Pixels without a chain go through
tests/_reproject_model.py's reproject unchanged."""
import numpy as np

from _reproject_model import overlay, reproject

f32 = np.float32


def _i32(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


def end_points(rays):
    """X = O + t * D per component of pt_read_through_rays' records (..., 8)"""
    rays = np.asarray(rays, f32)
    with np.errstate(all="ignore"):
        return rays[..., 0:3] + rays[..., 3:4] * rays[..., 4:7]


def reproject_through(rn, rh, sn, sh, yn, yh, frame, T, fin_h, fin_n, mat_vd, rot_h, max_history, depth_tol, normal_tol, point_tol, radius,
                      all_materials=False):
    """The new FRAME, the new T (None when T is None), the kept count, the kept count of the chain pixels, and info: "chain" (H, W) bool, k_p >= 1
    and not under the overlay; "guess" and "source" (H, W) int64 flat pixel indices, -1 where there is none.
    rn, rh: (H, W, 16) first-hit records under the current inputs fin_n / the image's camera fin_h; sn, sh: the seen-through records and
    yn, yh: (H, W, 8) their last segments, for the same two; frame, T: (H, W, 4) of the image; mat_vd: material_flags;
    rot_h: cam_rot(fin_h["rotation"])."""
    H, W = frame.shape[:2]
    n = H * W
    out, tout, _ = reproject(rn, rh, frame, T, fin_h, fin_n, mat_vd, rot_h, max_history, depth_tol, normal_tol, all_materials)      # 2
    out = out.reshape(n, 4).copy()
    tout = None if tout is None else tout.reshape(n, 4).copy()
    sn = np.ascontiguousarray(sn, f32).reshape(n, 16)
    sh = np.ascontiguousarray(sh, f32).reshape(n, 16)
    yn = np.ascontiguousarray(yn, f32).reshape(n, 8)
    yh = np.ascontiguousarray(yh, f32).reshape(n, 8)
    fr = np.ascontiguousarray(frame, f32).reshape(n, 4)
    Ts = None if T is None else np.ascontiguousarray(T, f32).reshape(n, 4)
    M = np.asarray(rot_h, f32)
    Oh, On = fin_h["origin"], fin_n["origin"]
    ss, fl, hr = f32(fin_h["params"][0]), f32(fin_h["params"][1]), f32(fin_h["params"][3])
    mat_vd = np.asarray(mat_vd, np.uint8)
    mh = f32(max_history)
    k = _i32(sn[:, 14])
    chain = (k >= 1) & ~overlay(W, H, fin_n).ravel()                                             # 1
    P = np.flatnonzero(chain)
    guess = np.full(n, -1, np.int64)
    source = np.full(n, -1, np.int64)
    with np.errstate(all="ignore"):
        # what a candidate s offers (the kernel's packed pixels)
        Xh = end_points(yh)
        wordh = _i32(sh[:, 11])
        Nh = sh[:, 1:4]
        usable = (_i32(sh[:, 7]) != -1) & np.isfinite(Xh).all(1) & (fr[:, 3] > 0) & np.isfinite(fr[:, :3]).all(1)
        S, Y = sn[P], yn[P]
        L, N, D0 = S[:, 0], S[:, 1:4], S[:, 8:11]
        word = _i32(S[:, 11])
        mat = word & 0xfff
        matok = mat < mat_vd.size
        vd = np.ones(P.size, bool)
        vd[matok] = mat_vd[mat[matok]] != 0
        ok = (_i32(S[:, 7]) != -1) & np.isfinite(L) & (L > 0) & np.isfinite(N).all(1) & np.isfinite(D0).all(1) & np.isfinite(Y[:, :7]).all(1)      # 3
        ok &= matok & (bool(all_materials) | ~vd)
        X = end_points(Y)
        V = On[None, :] + L[:, None] * D0                                                        # 4
        v = V - Oh[None, :]
        v0, v1, v2 = v[:, 0], v[:, 1], v[:, 2]
        q = [(v0 * M[3 * i] + v1 * M[3 * i + 1]) + v2 * M[3 * i + 2] for i in range(3)]
        a = (q[0] / q[2]) * fl
        b = (q[1] / q[2]) * fl
        sx = ((f32(1) - a / ss) * f32(0.5)) * f32(W)
        sy = ((f32(1) + b / (hr * ss)) * f32(0.5)) * f32(H)
        ok &= (q[2] > 0) & (sx >= 0) & (sx < f32(W)) & (sy >= 0) & (sy < f32(H))
        cx = np.where(ok, sx, 0).astype(np.int64)
        cy = np.where(ok, sy, 0).astype(np.int64)
        guess[P[ok]] = (cy * W + cx)[ok]
        tol = f32(point_tol) * L                                                                  # 5
        tol2 = tol * tol
        best = np.zeros(P.size, f32)
        src = np.full(P.size, -1, np.int64)
        for dy in range(-int(radius), int(radius) + 1):
            for dx in range(-int(radius), int(radius) + 1):
                x, y = cx + dx, cy + dy
                inside = ok & (x >= 0) & (x < W) & (y >= 0) & (y < H)
                s = np.where(inside, y * W + x, 0)
                e = Xh[s] - X
                d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
                dot = (N[:, 0] * Nh[s, 0] + N[:, 1] * Nh[s, 1]) + N[:, 2] * Nh[s, 2]
                take = inside & (wordh[s] == word) & usable[s] & (d2 <= tol2) & (dot >= f32(normal_tol)) & ((src < 0) | (d2 < best))
                best = np.where(take, d2, best)
                src = np.where(take, s, src)
        ok &= src >= 0
        source[P[ok]] = src[ok]
        F = fr[np.where(ok, src, 0)]                                                             # 6
        o = F.copy()
        cap = F[:, 3] > mh
        f = mh / F[:, 3]
        o[cap, :3] = F[cap, :3] * f[cap, None]
        o[cap, 3] = mh
        o[~ok] = 0
        out[P] = o
        if Ts is not None:
            Tq = Ts[np.where(ok, src, 0)]
            t = Tq.copy()
            tcap = Tq[:, 2] > mh
            g = mh / Tq[:, 2]
            t[tcap, 0] = Tq[tcap, 0] * g[tcap]
            t[tcap, 1] = Tq[tcap, 1] * g[tcap]
            t[tcap, 2] = mh
            t[~ok] = 0
            tout[P] = t
    kept = int((out[:, 3] > 0).sum())                                                            # a kept pixel has a count > 0
    info = {"chain": chain.reshape(H, W), "guess": guess.reshape(H, W), "source": source.reshape(H, W)}
    return out.reshape(H, W, 4), None if tout is None else tout.reshape(H, W, 4), kept, int(ok.sum()), info
