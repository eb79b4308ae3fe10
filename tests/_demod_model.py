"""A float32 numpy model of the albedo-demodulated calls of include/pt_demod.h, written from the header's text on top of the models of the plain
calls (tests/_guided_model.py, tests/_steer_model.py, tests/_reproject_model.py) (not a test module: the helpers of tests/test_demod_abi.py and
tests/test_gpu_demod.py)."""
import numpy as np

from _adaptive_model import select
from _denoise_model import H5, _inv, classify
from _guided_model import INF32, K3, _shift, lum, variance
from _reproject_model import reproject

f32 = np.float32


def demodulate(frame, feat, T, floor):
    """The filter-side quantities of the header: a dict of cls (with the pixels whose I is not finite made invalid), a, L, I (the filter's colour
    input: c / a on a valid hit, c elsewhere), T' and feat' (feat with those pixels marked invalid for the plain model's own classification)."""
    frame = np.asarray(frame, f32)
    feat = np.asarray(feat, f32)
    T = np.asarray(T, f32)
    c, cls = classify(frame, feat)
    hit = cls == 1
    with np.errstate(all="ignore"):
        a = np.where(hit[..., None], np.maximum(feat[..., 4:7], f32(floor)), f32(1)).astype(f32)
        I = np.where(hit[..., None], c / a, c).astype(f32)
        bad = hit & ~np.isfinite(I).all(-1)
        cls = np.where(bad, 0, cls)
        a = np.where(bad[..., None], f32(1), a).astype(f32)
        I = np.where(bad[..., None], c, I).astype(f32)
        L = np.where(cls == 1, lum(a), f32(1)).astype(f32)                 # exactly 1 off the valid hits, by definition
        Tp = T.copy()
        Tp[..., 0] = T[..., 0] / L
        Tp[..., 1] = (T[..., 1] / L) / L
    featx = feat.copy()
    featx[bad, 0] = np.nan                                                # a non-finite t: invalid for classify()
    return {"cls": cls, "a": a, "L": L, "I": I, "T": Tp, "feat": featx, "c": c}


def passes(c, v, cls, feat, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo):
    """include/pt_guided.h's passes 0 .. K-1 over a given (c, v) and classes: the loop of _guided_model.denoise_guided, which takes its input from
    FRAME alone (tests/test_demod_abi.py holds the two together bit for bit)"""
    feat = np.asarray(feat, f32)
    c = np.asarray(c, f32)
    v = np.asarray(v, f32)
    t, Nn, Kd = feat[..., 0], feat[..., 1:4], feat[..., 4:7]
    invN, invD, invA = _inv(1, sigma_normal), _inv(1, sigma_depth), _inv(1, sigma_albedo)
    sl = f32(sigma_lum)
    hitp = cls == 1
    valid = cls != 0
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            gs = np.zeros(cls.shape, f32); gw = np.zeros(cls.shape, f32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    use = valid & (_shift(cls, dy, dx, 0) == cls)
                    k = K3[dy + 1] * K3[dx + 1]
                    gs = np.where(use, gs + k * _shift(v, dy, dx, f32(0)), gs).astype(f32)
                    gw = np.where(use, gw + k, gw).astype(f32)
            g = gs / gw
            lum_on = np.isfinite(sl) & (g != INF32)
            den = sl * np.sqrt(g) + f32(1e-10)
            lp = lum(c)
            num = np.zeros(c.shape, f32); sw = np.zeros(cls.shape, f32); sv = np.zeros(cls.shape, f32)
            vinf = np.zeros(cls.shape, bool)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ddy, ddx = dy * s, dx * s
                    use = valid & (_shift(cls, ddy, ddx, 0) == cls)
                    cq = _shift(c, ddy, ddx, f32(0))
                    vq = _shift(v, ddy, ddx, f32(0))
                    e = np.where(lum_on, np.abs(lp - lum(cq)) / den, f32(0)).astype(f32)
                    dt = (t - _shift(t, ddy, ddx, f32(0))) / t
                    geo = ((Nn - _shift(Nn, ddy, ddx, f32(0))) ** 2).sum(-1, dtype=f32) * invN + (dt * dt) * invD + \
                        ((Kd - _shift(Kd, ddy, ddx, f32(0))) ** 2).sum(-1, dtype=f32) * invA
                    e = np.where(hitp, e + geo, e).astype(f32)
                    w = ((H5[dy + 2] * H5[dx + 2]) * np.exp(-e)).astype(f32)
                    use = use & ~(w < f32(1e-30))
                    w = np.where(use, w, f32(0)).astype(f32)
                    num += np.where(use[..., None], w[..., None] * cq, f32(0))
                    sw += w
                    tap_inf = use & (vq == INF32)
                    vinf |= tap_inf
                    sv = np.where(use & ~tap_inf, sv + (w * w) * vq, sv).astype(f32)
            c = np.where(valid[..., None], num / sw[..., None], c).astype(f32)
            v = np.where(valid, np.where(vinf, INF32, sv / (sw * sw)), v).astype(f32)
    return c, v


def filtered_demod(frame, feat, T, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames, floor):
    """(I_K, v_K, d): the filtered illumination, its carried variance and demodulate()'s dict"""
    d = demodulate(frame, feat, T, floor)
    v = variance(frame, d["feat"], d["T"], min_frames)                    # the plain rule on T': s2' / A, pooled over class and material
    I, v = passes(d["I"], v, d["cls"], feat, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo)
    return I, v, d


def denoise_guided_demod(frame, feat, T, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames, floor):
    """(H, W, 4) float32: rgb = a_p * I_K, a = FRAME.a"""
    frame = np.asarray(frame, f32)
    I, _, d = filtered_demod(frame, feat, T, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames, floor)
    with np.errstate(all="ignore"):
        rgb = (d["a"] * I).astype(f32)
    return np.concatenate([rgb, frame[..., 3:4]], axis=-1).astype(f32)


def select_guided_demod(frame, feat, T, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames, rel_err, abs_err=0.0, max_frames=0,
                        floor=0.01, overlay=None, detail=False):
    """the rule's (H, W) bool mask; detail: also the deciding step per pixel and step 5's two sides, v = (v_K * L) * L and tol^2"""
    frame = np.asarray(frame, f32)
    T = np.asarray(T, f32)
    n = T[..., 2]
    I, vK, d = filtered_demod(frame, feat, T, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames, floor)
    cls, L = d["cls"], d["L"]
    with np.errstate(all="ignore"):
        cK = (d["a"] * I).astype(f32)
        tol = np.fmax(f32(rel_err) * np.abs(lum(cK)), f32(abs_err)).astype(f32)
        tol2 = (tol * tol).astype(f32)
        v = np.where(cls == 1, (vK * L) * L, vK).astype(f32)
        guided = (vK == INF32) | (v > tol2)
    own = select(T, rel_err, abs_err, min_frames, 0)                     # steps 3 and 4 for the invalid pixels, on the raw T
    act = np.where(cls == 0, own, guided | (n < f32(min_frames)))
    step = np.where(cls == 0, 4, 5)
    step = np.where(n < f32(min_frames), 3, step)
    if max_frames > 0:
        cap = n >= f32(max_frames)
        act = act & ~cap
        step = np.where(cap, 2, step)
    if overlay is not None:
        act = act & ~overlay
        step = np.where(overlay, 1, step)
    if detail:
        return act, {"step": step, "v": v, "tol2": tol2}
    return act


def carried_albedo(rec, floor):
    """b of the header for (..., 16) feature records: the floored Kd of a hit (code != -1) with a finite Kd, else (1, 1, 1)"""
    rec = np.asarray(rec, f32)
    hit = np.ascontiguousarray(rec[..., 7]).view(np.int32) != -1
    Kd = rec[..., 4:7]
    use = hit & np.isfinite(Kd).all(-1)
    with np.errstate(all="ignore"):
        return np.where(use[..., None], np.maximum(Kd, f32(floor)), f32(1)).astype(f32)


def reproject_demod(rn, rh, frame, T, fin_h, fin_n, mat_vd, rot_h, max_history, depth_tol, normal_tol, all_materials=False, floor=0.01):
    """The new FRAME, the new T (None when T is None) and the kept count.  Steps 1-6 are the plain model's: which pixels are kept is read off its
    result, and the source pixel s off its result on an image of pixel indices; step 7 is the header's."""
    H, W = frame.shape[:2]
    n = H * W
    fr = np.ascontiguousarray(frame, f32).reshape(n, 4)
    plain, _, kept = reproject(rn, rh, frame, None, fin_h, fin_n, mat_vd, rot_h, max_history, depth_tol, normal_tol, all_materials)
    ok = plain.reshape(n, 4)[:, 3] > 0                                    # a kept pixel has F.a > 0, capped or not
    assert n < (1 << 24)                                                  # float32 holds every pixel index
    idx = np.zeros((H, W, 4), f32)
    idx[..., 0] = np.arange(n, dtype=f32).reshape(H, W)
    idx[..., 3] = 1
    src, _, _ = reproject(rn, rh, idx, None, fin_h, fin_n, mat_vd, rot_h, np.inf, depth_tol, normal_tol, all_materials)
    s = np.where(ok, src.reshape(n, 4)[:, 0], 0).astype(np.int64)
    bn = carried_albedo(np.ascontiguousarray(rn, f32).reshape(n, 16), floor)
    bh = carried_albedo(np.ascontiguousarray(rh, f32).reshape(n, 16), floor)[s]
    mh = f32(max_history)
    with np.errstate(all="ignore"):
        r = bn / bh
        rho = lum(bn) / lum(bh)
        F = fr[s]
        out = F.copy()
        out[:, :3] = F[:, :3] * r
        cap = F[:, 3] > mh
        f = mh / F[:, 3]
        out[cap, :3] = out[cap, :3] * f[cap, None]
        out[cap, 3] = mh
        out[~ok] = 0
        tout = None
        if T is not None:
            Ts = np.ascontiguousarray(T, f32).reshape(n, 4)[s]
            tout = Ts.copy()
            tout[:, 0] = Ts[:, 0] * rho
            tout[:, 1] = (Ts[:, 1] * rho) * rho
            tcap = Ts[:, 2] > mh
            g = mh / Ts[:, 2]
            tout[tcap, 0] = tout[tcap, 0] * g[tcap]
            tout[tcap, 1] = tout[tcap, 1] * g[tcap]
            tout[tcap, 2] = mh
            tout[~ok] = 0
            tout = tout.reshape(H, W, 4)
    assert int(ok.sum()) == kept
    return out.reshape(H, W, 4), tout, kept
