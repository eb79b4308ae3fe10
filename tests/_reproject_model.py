"""float32 model of the reprojection of include/pt_reproject.h: the mapping, step by step, in the header's order (numpy float32 rounds every
operation as binary32, with no contraction), so that tests/test_gpu_reproject.py can hold the device to it bit for bit."""
import numpy as np

f32 = np.float32


def frame_in(params, origin, rotation, mouse=(-1.0e6, -1.0e6, 0.0)):
    """the frame inputs of one image: Parameters (12), ORIGIN, ROTATION, MOUSE_POS as float32 arrays"""
    return {"params": np.asarray(params, f32)[:12], "origin": np.asarray(origin, f32)[:3], "rotation": np.asarray(rotation, f32)[:3],
            "mouse": np.asarray(mouse, f32)[:3]}


def cam_rot(rotation, cos=None, sin=None):
    """camRot = rotateX * rotateY * (z != 0 ? rotateZ : I), row-major, as k_frame_setup builds it.  cos / sin: the shader's functions over
    float32 arrays (Renderer.debug_math("cos" / "sin") on the GPU); numpy's by default, which agree on the angles 0 and the hand-made cases."""
    cos = cos or (lambda x: np.cos(np.asarray(x, f32)).astype(f32))
    sin = sin or (lambda x: np.sin(np.asarray(x, f32)).astype(f32))
    ax, ay, az = (f32(v) for v in rotation)
    c = cos(np.array([ax, ay, az], f32)); s = sin(np.array([ax, ay, az], f32))
    cx, sx, cy, sy = c[0], s[0], c[1], s[1]
    one, zero = f32(1), f32(0)
    RX = [one, zero, zero, zero, cx, sx, zero, -sx, cx]
    RY = [cy, zero, -sy, zero, one, zero, sy, zero, cy]
    RZ = [one, zero, zero, zero, one, zero, zero, zero, one]
    if az != 0:
        cz, sz = c[2], s[2]
        RZ[0], RZ[1], RZ[3], RZ[4] = cz, sz, -sz, cz

    def mul(A, B):
        return [f32(f32(f32(A[3 * i] * B[j]) + f32(A[3 * i + 1] * B[3 + j])) + f32(A[3 * i + 2] * B[6 + j])) for i in range(3) for j in range(3)]
    return np.array(mul(mul(RX, RY), RZ), f32)


def material_flags(mtl):
    """one flag per material of a MATERIALS buffer (binding 14): 1 = view-dependent (Pr != 1, Pc != 0, Tr > 0, Tf[0] > 0, illum 5 or 7, or a
    map_Pr, map_Pc or map_Tr >= 0), as buildScene reads the 48-float records"""
    mtl = np.asarray(mtl, f32)
    me = int(mtl[0])
    n = (mtl.size - 1) // me
    out = np.zeros(max(n, 1), np.uint8)
    for m in range(n):
        F = mtl[me * m: me * m + me]
        illum = int(F[21])
        out[m] = int(F[26] != 1 or F[28] != 0 or F[12] > 0 or F[13] > 0 or illum in (5, 7) or int(F[33]) >= 0 or int(F[35]) >= 0 or int(F[39]) >= 0)
    return out[:n] if n else out[:0]


def overlay(W, H, fin):
    """the pixels under MOUSE_POS's overlay (pt_device.hpp inMouseOverlay, frag.glsl:888): (H, W) bool"""
    half = f32(fin["params"][2]) * f32(0.005)
    ys, xs = np.mgrid[0:H, 0:W]
    return (np.abs(xs.astype(f32) - fin["mouse"][0]) < half) & (np.abs(ys.astype(f32) - fin["mouse"][1]) < half)


def reproject(rn, rh, frame, T, fin_h, fin_n, mat_vd, rot_h, max_history, depth_tol, normal_tol, all_materials=False):
    """The new FRAME, the new T (None when T is None) and the kept count.  rn, rh: (H, W, 16) feature records under the current inputs fin_n / the
    image's camera fin_h; frame, T: (H, W, 4) of the image; mat_vd: material_flags; rot_h: cam_rot(fin_h["rotation"])."""
    H, W = frame.shape[:2]
    n = H * W
    rn = np.ascontiguousarray(rn, f32).reshape(n, 16)
    rh = np.ascontiguousarray(rh, f32).reshape(n, 16)
    fr = np.ascontiguousarray(frame, f32).reshape(n, 4)
    M = np.asarray(rot_h, f32)
    Oh, On = fin_h["origin"], fin_n["origin"]
    ss, fl, hr = f32(fin_h["params"][0]), f32(fin_h["params"][1]), f32(fin_h["params"][3])
    mat_vd = np.asarray(mat_vd, np.uint8)
    with np.errstate(all="ignore"):
        t, N, D = rn[:, 0], rn[:, 1:4], rn[:, 8:11]
        code, mat = rn[:, 7].copy().view(np.int32), rn[:, 11].copy().view(np.int32)
        hit = code != -1                                                                          # 2
        matok = (mat >= 0) & (mat < mat_vd.size)
        vd = np.ones(n, bool)
        vd[matok] = mat_vd[mat[matok]] != 0
        ok = np.where(hit, np.isfinite(t) & np.isfinite(N).all(1) & np.isfinite(D).all(1) & matok & (bool(all_materials) | ~vd), True)
        P = On[None, :] + t[:, None] * D
        v = np.where(hit[:, None], P - Oh[None, :], D)
        v0, v1, v2 = v[:, 0], v[:, 1], v[:, 2]
        q = [(v0 * M[3 * i] + v1 * M[3 * i + 1]) + v2 * M[3 * i + 2] for i in range(3)]       # 3
        a = (q[0] / q[2]) * fl                                                                   # 4
        b = (q[1] / q[2]) * fl
        sx = ((f32(1) - a / ss) * f32(0.5)) * f32(W)
        sy = ((f32(1) + b / (hr * ss)) * f32(0.5)) * f32(H)
        ok &= (q[2] > 0) & (sx >= 0) & (sx < f32(W)) & (sy >= 0) & (sy < f32(H))
        s = np.where(ok, np.where(ok, sy, 0).astype(np.int64) * W + np.where(ok, sx, 0).astype(np.int64), 0)
        h = rh[s]                                                                                # 5
        ht, hN = h[:, 0], h[:, 1:4]
        hhit = h[:, 7].copy().view(np.int32) != -1
        hmat = h[:, 11].copy().view(np.int32)
        ln = np.sqrt((v0 * v0 + v1 * v1) + v2 * v2)
        dot = (N[:, 0] * hN[:, 0] + N[:, 1] * hN[:, 1]) + N[:, 2] * hN[:, 2]
        hitok = hhit & (hmat == mat) & np.isfinite(ht) & (ht > 0) & (np.abs(ln - ht) <= f32(depth_tol) * ht) & (dot >= f32(normal_tol))
        ok &= np.where(hit, hitok, ~hhit)
        F = fr[s]                                                                                # 6
        ok &= (F[:, 3] > 0) & np.isfinite(F[:, :3]).all(1)
        ok &= ~overlay(W, H, fin_n).ravel()                                                      # 1
        mh = f32(max_history)
        out = F.copy()                                                                           # 7
        cap = F[:, 3] > mh
        f = mh / F[:, 3]
        out[cap, :3] = F[cap, :3] * f[cap, None]
        out[cap, 3] = mh
        out[~ok] = 0
        tout = None
        if T is not None:
            Ts = np.ascontiguousarray(T, f32).reshape(n, 4)[s]
            tout = Ts.copy()
            tcap = Ts[:, 2] > mh
            g = mh / Ts[:, 2]
            tout[tcap, 0] = Ts[tcap, 0] * g[tcap]
            tout[tcap, 1] = Ts[tcap, 1] * g[tcap]
            tout[tcap, 2] = mh
            tout[~ok] = 0
            tout = tout.reshape(H, W, 4)
    return out.reshape(H, W, 4), tout, int(ok.sum())
