"""A float32 model of the chain of include/pt_through.h, written from the header's text over a rayScene callable (oracle.ray_scene, or a hand-made
scene), operation order as oracle/glsl_math.h (not a test module: the helper of tests/test_through_abi.py and tests/test_gpu_through.py).

Every operation is a binary32 +, -, *, /, sqrt or an exactly rounded fused multiply-add (fma below: the float64 sum rounded to odd, then to
binary32).  `exact_dirs=True` recomputes the two directions of step 7 in float64 from the same inputs and rounds them: a chain that changes under it
hangs on the last bits of a direction, which is what the GPU test may exclude."""
import struct

import numpy as np

f32 = np.float32
REFLECT, TRANSMIT, KEY = 1, 2, 1
MAPS = (22, 23, 24, 32, 33, 35, 37, 39, 41)                 # map_Ka, Kd, Ks, Pm, Pr, Pc, norm, Tr, Ke of the 48-float material record
EDGE = 1e-5                                                 # a weight this close to a threshold of step 6 is a fragile decision


def fma(a, b, c):
    """binary32 fma(a, b, c), exactly rounded: the product of two binary32 is exact in float64; the sum is rounded to odd there (TwoSum gives the
    error's sign), which makes the second rounding to binary32 the rounding of the exact value"""
    p = float(a) * float(b)
    c = float(c)
    s = p + c
    if not np.isfinite(s) or s == 0.0:
        return f32(s)
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    if e != 0.0 and not (struct.unpack("<Q", struct.pack("<d", s))[0] & 1):
        s = float(np.nextafter(s, np.inf if e > 0 else -np.inf))
    return f32(s)


def v3(x, y, z):
    return [f32(x), f32(y), f32(z)]


def dot(a, b):
    return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0]))


def cross(a, b):
    return [fma(a[1], b[2], -(a[2] * b[1])), fma(a[2], b[0], -(a[0] * b[2])), fma(a[0], b[1], -(a[1] * b[0]))]


def madd(a, s, b):
    return [fma(a[k], s, b[k]) for k in range(3)]


def reflect(I, N):
    k = f32(2) * dot(N, I)
    return madd(N, -k, I)


def refract(I, N, eta):
    d = dot(N, I)
    k = f32(1) - eta * eta * (f32(1) - d * d)
    if k < 0:
        return v3(0, 0, 0)
    s = fma(eta, d, np.sqrt(k))
    return madd(N, -s, [I[j] * eta for j in range(3)])


def _reflect64(I, N):
    I, N = np.asarray(I, np.float64), np.asarray(N, np.float64)
    return list((I - 2.0 * np.dot(N, I) * N).astype(f32))


def _refract64(I, N, n1, n2):
    I, N = np.asarray(I, np.float64), np.asarray(N, np.float64)
    eta = float(n1) / float(n2)
    d = np.dot(N, I)
    k = 1.0 - eta * eta * (1.0 - d * d)
    if not k >= 0:
        return v3(0, 0, 0) if k < 0 else v3(np.nan, np.nan, np.nan)
    return list((eta * I - (eta * d + np.sqrt(k)) * N).astype(f32))


def fresnel(n1, n2, normal, incidence):
    r0 = (n1 - n2) / (n1 + n2)
    r0 = r0 * r0
    cosX = -dot(normal, incidence)
    if n1 > n2:
        n = n1 / n2
        sinT2 = n * n * (f32(1) - cosX * cosX)
        if sinT2 > 1:
            return f32(1)
        cosX = np.sqrt(f32(1) - sinT2)
    x = f32(1) - cosX
    return r0 + (f32(1) - r0) * x * x * x * x * x


def sample_tex(tex, u, v):
    """oracle sampleTex: LINEAR / REPEAT on RGBA8"""
    h, w = tex.shape[:2]
    fu, fv = f32(u) * f32(w) - f32(0.5), f32(v) * f32(h) - f32(0.5)
    flu = np.floor(fu) if abs(fu) < 1e9 else f32(0)
    flv = np.floor(fv) if abs(fv) < 1e9 else f32(0)
    a, b = fu - flu, fv - flv
    i0, j0 = int(flu) % w, int(flv) % h
    i1, j1 = (i0 + 1) % w, (j0 + 1) % h
    one = f32(1)
    w00, w10, w01, w11 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
    t = lambda j, i: f32(tex[j, i, :3]) / f32(255)
    return list(w00 * t(j0, i0) + w10 * t(j0, i1) + w01 * t(j1, i0) + w11 * t(j1, i1))


def tri_uv(tris, tri, o, d):
    """hit.uvSample of a triangle hit: rayTri's (u, v) on the offset origin (frag.glsl:549), then :508-517"""
    T = tris[40 * tri: 40 * tri + 40]
    if T[24] == f32(69.420):
        return f32(-1), f32(-1)
    o = madd(d, f32(1e-4), o)
    v1 = list(T[0:3])
    e1 = [T[4 + k] - T[k] for k in range(3)]
    e2 = [T[8 + k] - T[k] for k in range(3)]
    dxe2 = cross(d, e2)
    inv = f32(1) / dot(e1, dxe2)
    s = [o[k] - v1[k] for k in range(3)]
    u = dot(s, dxe2) * inv
    v = dot(d, cross(s, e1)) * inv
    w = f32(1) - u - v
    uvx = T[28] * u + T[32] * v + w * T[24]
    uvy = T[29] * u + T[33] * v + w * T[25]
    return uvx, f32(1) - uvy


def materials(mtl):
    m = np.asarray(mtl, f32).reshape(-1)
    me = int(m[0])
    return [m[me * k: me * k + me] for k in range((m.size - 1) // me)]


def _finite3(v):
    return all(np.isfinite(float(x)) for x in v)


def chain(ray, mats, O, D0, max_depth, min_weight, lobes, flags, raytracing=True, textures=None, tris=None, exact_dirs=False):
    """The chain of one pixel.  ray(o, d) -> (hit code or < 0, out[8] = t, loc, N, material) is rayScene.  Returns a dict: rec (16 float32, the
    record S), ray (8 float32, pt_read_through_rays' entry), k, codes (the hit code of every surface met), margin (the smallest distance of a weight
    from a threshold it was compared with), last_dir (D of the recorded segment).  textures / tris: needed by scenes with mapped materials (uv)."""
    one = f32(1)
    O, D = [f32(x) for x in O], [f32(x) for x in D0]
    D0 = list(D)
    stack, size = [f32(0)] * 10, 0
    stack[0], size = f32(1.0029), 1
    tint, L, k, first = [one, one, one], f32(0), 0, -1
    rec = np.zeros(16, f32)
    rec[0] = -1
    rec[7] = np.int32(-1).view(f32)
    rec[8:11] = D0
    rec[11] = np.int32(-1).view(f32)
    out_ray = np.array(O + [f32(-1)] + D + [np.int32(0).view(f32)], f32)
    codes, margin = [], np.inf
    depth = max_depth if (lobes and raytracing) else 0
    min_weight = f32(min_weight)
    with np.errstate(all="ignore"):
        while True:
            code, out = ray(O, D)
            if code < 0:
                break
            codes.append(int(code))
            t, loc, N, mat = f32(out[0]), [f32(x) for x in out[1:4]], [f32(x) for x in out[4:7]], int(out[7])
            m = np.array(mats[mat], f32)
            uvx = uvy = f32(0)
            if tris is not None and (code >> 24) == 1:
                uvx, uvy = tri_uv(tris, code & 0xFFFFFF, O, D)
            if any(m[j] > -1 for j in MAPS):
                if (code >> 24) != 1 or tris is None:
                    raise NotImplementedError("a mapped material on an ellipsoid, or no triangle buffer for the uv")
                tx = lambda j: sample_tex(textures[int(m[j])], uvx, uvy)
                if m[23] > -1:
                    m[4:7] = np.array(tx(23), f32) * m[4:7]
                if m[39] > -1:
                    m[12] = tx(39)[0]
                if m[32] > -1:
                    m[25] = tx(32)[0]
                if m[33] > -1:
                    m[26] = tx(33)[0]
                if m[35] > -1:
                    m[28] = tx(35)[0]
                if m[37] > -1:
                    N = [f32(x) for x in tx(37)]
            L = L + t
            Kd = [m[4], m[5], m[6]]
            through = [tint[j] * Kd[j] for j in range(3)]
            if k == 0:
                first = mat
            word = mat if (k == 0 or not (flags & KEY)) else (k << 24) | (first << 12) | mat
            rec[0] = L
            rec[1:4] = N
            rec[4:7] = through
            rec[7] = np.int32(code).view(f32)
            rec[11] = np.int32(word).view(f32)
            rec[12], rec[13] = uvx, uvy
            rec[14] = np.int32(k).view(f32)
            out_ray = np.array(O + [t] + D + [np.int32(k).view(f32)], f32)
            if k >= depth:
                break
            ND = dot(N, D)
            Nf = [x * (f32(-1) if ND > 0 else one) for x in N]
            if ND < 0:                                        # addToIndiceStack (frag.glsl:139-147), then n1 = stack[1], n2 = stack[0]
                if size < 10:
                    for i in range(size, 0, -1):
                        stack[i] = stack[i - 1]
                    stack[0] = m[16]
                    size += 1
                n1, n2 = stack[1], stack[0]
            else:
                n1, n2 = stack[0], stack[1]
                if size > 0:
                    for i in range(size - 1):
                        stack[i] = stack[i + 1]
                    size -= 1
            r = one - m[26]
            c = m[28]
            tw = m[12] if m[12] > 0 else ((m[13] + m[14] + m[15]) / f32(3) if m[13] > 0 else f32(0))
            fr = f32(0)
            if int(m[21]) in (5, 7) or tw > 0:
                fr = fresnel(n1, n2, Nf, D)
                r = r + fr * m[26]
                tw = tw * (one - fr)
            d = (one - m[25]) * (one - tw) * (one - fr)
            total = d + r + c + tw
            r, tw = r / total, tw / total
            nd = None
            if lobes & REFLECT:
                margin = min(margin, abs(float(r) - float(min_weight)))
                if r >= min_weight:
                    margin = min(margin, abs(float(r) - float(tw)))
            if (lobes & REFLECT) and r >= min_weight and r >= tw:
                nd = _reflect64(D, Nf) if exact_dirs else reflect(D, Nf)
            else:
                if lobes & TRANSMIT:
                    margin = min(margin, abs(float(tw) - float(min_weight)))
                if (lobes & TRANSMIT) and tw >= min_weight:
                    nd = _refract64(D, Nf, n1, n2) if exact_dirs else refract(D, Nf, n1 / n2)
            if nd is None or not _finite3(nd) or all(x == 0 for x in nd):
                break
            tint, O, D, k = through, loc, [f32(x) for x in nd], k + 1
    if np.isnan(margin):
        margin = 0.0
    return {"rec": rec, "ray": out_ray, "k": int(np.float32(rec[14]).view(np.int32)), "codes": codes, "margin": margin, "last_dir": out_ray[4:7].copy()}


def through_features(oracle, wl, dirs, max_depth, min_weight, lobes, flags, uv=False, fragile=False, pixels=None):
    """The records S of a workload along the lens-centre directions `dirs` (H, W, 3), over the oracle's rayScene: (feat (H, W, 16), rays (H, W, 8),
    info).  uv: fill S3's uv from the triangle buffer (the first-hit model of tests/test_fill_abi.py leaves it 0).  fragile: also info["fragile"],
    the pixels whose decisions lie within EDGE of a threshold or whose chain changes under exact_dirs.  pixels: flat indices to compute (others 0)."""
    h, w = dirs.shape[:2]
    mats = materials(wl.buffers[14])
    sc = oracle.Scene.from_workload(wl)
    org = np.asarray(wl.buffers[0], f32)
    P = np.asarray(wl.buffers[4], f32)
    mapped = any(m[j] > -1 for m in mats for j in MAPS)
    tris = np.asarray(wl.buffers[3], f32).reshape(-1) if (uv or mapped) else None
    textures = getattr(wl, "textures", None)
    ray = lambda o, d: oracle.ray_scene(sc, o, d)
    feat, rays = np.zeros((h, w, 16), f32), np.zeros((h, w, 8), f32)
    frag = np.zeros((h, w), bool)
    for p in (range(h * w) if pixels is None else pixels):
        y, x = divmod(int(p), w)
        kw = dict(raytracing=bool(P[9] == 1), textures=textures, tris=tris)
        c = chain(ray, mats, org, dirs[y, x], max_depth, min_weight, lobes, flags, **kw)
        feat[y, x], rays[y, x] = c["rec"], c["ray"]
        if fragile:
            e = chain(ray, mats, org, dirs[y, x], max_depth, min_weight, lobes, flags, exact_dirs=True, **kw)
            frag[y, x] = c["margin"] < EDGE or e["codes"] != c["codes"] or e["k"] != c["k"]
    return feat, rays, {"fragile": frag}
