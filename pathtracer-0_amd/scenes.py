"""Synthetic workloads C1..C5 of BASELINE.json / SURVEY.md §8(d).

No asset of the reference is usable (all live under C:\\Graphics\\... off-repo,
/root/reference/src/Main/dispatch.java:221-257), so every workload is generated here,
deterministically, as OBJ text + scene-DSL calls and pushed through the same host-side producers a
reference user would call (hostlib.Scene == the reference's `scene` class).  All meshes carry
explicit `vn`, every OBJ starts with an `o` line (Q-14) and every `o` group has
at least two separable triangles (Q-16).
"""
import math

import numpy as np

from . import hostlib

# (W, H, spp, bounces) per BASELINE.json config
CONFIGS = {
    "C1": dict(W=256, H=256, spp=4, bounces=4, sample_res=4),
    "C2": dict(W=1280, H=720, spp=64, bounces=8, sample_res=8),
    "C3": dict(W=1920, H=1080, spp=256, bounces=8, sample_res=8),
    "C4": dict(W=1920, H=1080, spp=1024, bounces=8, sample_res=8),
    "C5": dict(W=3840, H=2160, spp=4096, bounces=16, sample_res=8),
    # not a BASELINE config: the shape of the reference author's own scenes (multi-group OBJs + addEllipsoid, dispatch.java:245-264)
    "C6": dict(W=1920, H=1080, spp=256, bounces=8, sample_res=8),
}


def frame_seed(f):
    """u_seed of frame f; stays inside the reference's [0,10000) (dispatch.java:698)."""
    return (1234 + 7919 * f) % 10000


def make_params(W, H, sample_res=8, max_bounces=8, blur=0.001, focal_distance=1.0, auto_focus=1.0, screen_size=1.5, focal_length=1.0):
    """Parameters block, dispatch.java:191-205 <-> frag.glsl:39-52."""
    return np.array([screen_size, focal_length, W, H / float(W), sample_res, max_bounces, 0.0, blur, focal_distance, 1.0, 0.0, auto_focus], dtype=np.float32)


# ---------------------------------------------------------------------------------- OBJ writer
class Obj:
    def __init__(self):
        self.lines = []
        self.nv = 0
        self.nn = 0

    def group(self, name):
        self.lines.append(f"o {name}")

    def usemtl(self, name):
        self.lines.append(f"usemtl {name}")

    def v(self, p):
        self.lines.append("v %.9g %.9g %.9g" % tuple(p))
        self.nv += 1
        return self.nv

    def vn(self, n):
        self.lines.append("vn %.9g %.9g %.9g" % tuple(n))
        self.nn += 1
        return self.nn

    def vt(self, uv):
        self.lines.append("vt %.9g %.9g" % tuple(uv))
        self.nt = getattr(self, "nt", 0) + 1
        return self.nt

    def f(self, a, b, c, na, nb=None, nc=None):
        nb = na if nb is None else nb
        nc = na if nc is None else nc
        self.lines.append(f"f {a}//{na} {b}//{nb} {c}//{nc}")

    def quad(self, p0, p1, p2, p3, n):
        i = [self.v(p) for p in (p0, p1, p2, p3)]
        k = self.vn(n)
        self.f(i[0], i[1], i[2], k)
        self.f(i[0], i[2], i[3], k)

    def quad_uv(self, p0, p1, p2, p3, n, uv0=(0.05, 0.05), uv1=(0.95, 0.95)):
        """quad with texture coordinates (first vt.y must not be 0: the packer reads that as "no uv")"""
        i = [self.v(p) for p in (p0, p1, p2, p3)]
        k = self.vn(n)
        t = []
        for (a, b) in ((uv0[0], uv0[1]), (uv1[0], uv0[1]), (uv1[0], uv1[1]), (uv0[0], uv1[1])):
            self.lines.append("vt %.9g %.9g" % (a, b))
            self.nt = getattr(self, "nt", 0) + 1
            t.append(self.nt)
        self.lines.append(f"f {i[0]}/{t[0]}/{k} {i[1]}/{t[1]}/{k} {i[2]}/{t[2]}/{k}")
        self.lines.append(f"f {i[0]}/{t[0]}/{k} {i[2]}/{t[2]}/{k} {i[3]}/{t[3]}/{k}")

    def box(self, center, half, yrot):
        """axis-aligned box of half extents `half` rotated by yrot about +y, 12 triangles, flat normals."""
        c, s = math.cos(yrot), math.sin(yrot)

        def R(p):
            return (c * p[0] + s * p[2], p[1], -s * p[0] + c * p[2])

        def P(x, y, z):
            q = R((x * half[0], y * half[1], z * half[2]))
            return (q[0] + center[0], q[1] + center[1], q[2] + center[2])

        faces = [((1, 0, 0), [(1, -1, -1), (1, 1, -1), (1, 1, 1), (1, -1, 1)]), ((-1, 0, 0), [(-1, -1, 1), (-1, 1, 1), (-1, 1, -1), (-1, -1, -1)]),
                 ((0, 1, 0), [(-1, 1, -1), (-1, 1, 1), (1, 1, 1), (1, 1, -1)]), ((0, -1, 0), [(-1, -1, 1), (-1, -1, -1), (1, -1, -1), (1, -1, 1)]),
                 ((0, 0, 1), [(1, -1, 1), (1, 1, 1), (-1, 1, 1), (-1, -1, 1)]), ((0, 0, -1), [(-1, -1, -1), (-1, 1, -1), (1, 1, -1), (1, -1, -1)])]
        for n, corners in faces:
            self.quad(*[P(*q) for q in corners], R(n))

    def mesh(self, verts, normals, faces):
        base_v, base_n = self.nv, self.nn
        for p in verts:
            self.v(p)
        for n in normals:
            self.vn(n)
        for a, b, c in faces:
            self.lines.append(f"f {a+1+base_v}//{a+1+base_n} {b+1+base_v}//{b+1+base_n} {c+1+base_v}//{c+1+base_n}")

    def text(self):
        return "\n".join(self.lines) + "\n"


def icosphere(subdiv, center, radius):
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    # tilt the unit sphere slightly so that no vertex normal has an exactly-zero component
    # (such normals take the flat-normal branch of frag.glsl:501)
    ax, ay = 0.1234, 0.2345
    Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    n = [Ry @ (Rx @ p) for p in v]
    verts = [tuple(np.array(center) + radius * q) for q in n]
    return verts, [tuple(q) for q in n], f


def displaced_torus(nu, nv_, center, R, r, amp, seed):
    """~2*nu*nv triangles; radial displacement = seeded sum of sines; normals from the analytic torus."""
    rs = np.random.RandomState(seed)
    ku, kv, ph = rs.randint(1, 9, size=6), rs.randint(1, 9, size=6), rs.uniform(0, 2 * math.pi, size=6)
    verts, normals, faces = [], [], []
    for i in range(nu):
        u = 2 * math.pi * i / nu
        for j in range(nv_):
            w = 2 * math.pi * j / nv_
            d = sum(math.sin(ku[k] * u + kv[k] * w + ph[k]) for k in range(6)) / 6.0
            rr = r * (1.0 + amp * d)
            n = (math.cos(w) * math.cos(u), math.sin(w), math.cos(w) * math.sin(u))
            p = ((R + rr * math.cos(w)) * math.cos(u), rr * math.sin(w), (R + rr * math.cos(w)) * math.sin(u))
            verts.append((p[0] + center[0], p[1] + center[1], p[2] + center[2]))
            normals.append(n)
    for i in range(nu):
        for j in range(nv_):
            a, b = i * nv_ + j, ((i + 1) % nu) * nv_ + j
            c, d = ((i + 1) % nu) * nv_ + (j + 1) % nv_, i * nv_ + (j + 1) % nv_
            faces += [(a, b, c), (a, c, d)]
    return verts, normals, faces


# ---------------------------------------------------------------------------------- scenes
class Workload:
    """Everything the render call consumes: SSBO contents by binding point + texture 0 + config."""

    def __init__(self, name, W, H, buffers, sky, sample_res, max_bounces, info, textures=None):
        self.name, self.W, self.H = name, W, H
        self.buffers = buffers            # {binding: np.ndarray}: 0,1,2,3,4,5,7,10,11,12,13,14
        self.sky = sky                    # (h, w, 4) uint8, texture index 0
        self.textures = dict(textures or {})   # {index >= 1: (h, w, 4) uint8}: the rest of the bindless table (binding 15)
        self.sample_res, self.max_bounces = sample_res, max_bounces
        self.info = info

    def with_params(self, **kw):
        p = self.buffers[4].copy()
        names = ["screenSize", "focalLength", "resolution", "screenHratio", "SAMPLE_RES", "MAX_BOUNCES", "GAMMA", "BLUR", "FOCAL_DISTANCE", "RAYTRACING", "DEBUG", "AUTO_FOCUS"]
        for k, v in kw.items():
            p[names.index(k)] = v
        b = dict(self.buffers)
        b[4] = p
        return Workload(self.name, self.W, self.H, b, self.sky, int(p[4]), int(p[5]), self.info, self.textures)


GPU_BVH = None          # set to a device index to build every workload's BVHs with pt_build_bvh (libpt_hip.so) instead of the CPU builder


def _new_scene():
    sc = hostlib.Scene()
    if GPU_BVH is not None:
        sc.use_gpu_bvh_builder(GPU_BVH)
    return sc


def _finish(name, sc, W, H, cam, rot, sky_rgb, sample_res, max_bounces, **pk):
    bufs = sc.pack()
    bufs[0] = np.array(cam, dtype=np.float32)
    bufs[1] = np.array(rot, dtype=np.float32)
    bufs[2] = np.array([-1.0e6, -1.0e6, 0.0], dtype=np.float32)      # MOUSE_POS off-screen (frag.glsl:888)
    bufs[4] = make_params(W, H, sample_res, max_bounces, **pk)
    sky = np.array(sky_rgb, dtype=np.uint8)
    if sky.ndim == 1:
        sky = np.array([[list(sky_rgb) + [255]]], dtype=np.uint8)
    info = dict(triangles=sc.count("triangles"), nodes=sc.count("nodes"), objects=sc.count("objects"), max_depth=sc.count("max_depth"),
                max_leaf=sc.count("max_leaf"), materials=sc.count("materials"), ellipsoids=sc.count("ellipsoids"))
    return Workload(name, W, H, bufs, sky, sample_res, max_bounces, info)


def _cornell_materials(sc):
    """white/red/green diffuse, light Ke=15. Names carry no directory suffix (parentDirectory="")."""
    idx = {}
    for name, kd in (("white", (0.73, 0.73, 0.73)), ("red", (0.65, 0.05, 0.05)), ("green", (0.12, 0.45, 0.15))):
        idx[name] = sc.addMaterial(name)
        sc.setLastMtl("Kd", kd)
        sc.setLastMtl("Pr", 1)
    idx["light"] = sc.addMaterial("light")
    sc.setLastMtl("Kd", (0.78, 0.78, 0.78))
    sc.setLastMtl("Ke", (15, 15, 15))
    return idx


def _cornell_room(o, boxes=True, light_dx=0.0):
    # room: x in [-1,1], y in [0,2], z in [-1,1]; open towards -z (camera side); light_dx slides the light quad along x
    o.group("walls")
    o.usemtl("white")
    o.quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, 1, 0))          # floor
    o.quad((-1, 2, -1), (-1, 2, 1), (1, 2, 1), (1, 2, -1), (0, -1, 0))         # ceiling
    o.quad((-1, 0, 1), (1, 0, 1), (1, 2, 1), (-1, 2, 1), (0, 0, -1))           # back
    o.usemtl("red")
    o.quad((1, 0, -1), (1, 2, -1), (1, 2, 1), (1, 0, 1), (-1, 0, 0))           # +x wall (image left: x is mirrored, frag.glsl:894)
    o.usemtl("green")
    o.quad((-1, 0, -1), (-1, 0, 1), (-1, 2, 1), (-1, 2, -1), (1, 0, 0))        # -x wall
    o.group("light")
    o.usemtl("light")
    o.quad((-0.25 + light_dx, 1.98, -0.25), (0.25 + light_dx, 1.98, -0.25), (0.25 + light_dx, 1.98, 0.25), (-0.25 + light_dx, 1.98, 0.25), (0, -1, 0))
    if boxes:
        o.group("tallbox")
        o.usemtl("white")
        o.box((0.35, 0.6, 0.3), (0.3, 0.6, 0.3), 0.3)
        o.group("shortbox")
        o.usemtl("white")
        o.box((-0.35, 0.3, -0.3), (0.3, 0.3, 0.3), -0.3)


CORNELL_CAM = (0.0, 1.0, -1.6)
CORNELL_ROT = (0.0, 0.0, 0.0)


def c1_spheres(W=256, H=256, sample_res=4, max_bounces=4):
    """C1 'built-in sphere scene': 3 addEllipsoid over a ground quad (pattern of dispatch.java:245,264), 1x1 sky."""
    sc = _new_scene()
    sc.addMaterial("default")
    sc.setLastMtl("Kd", (0.8, 0.8, 0.8))
    sc.setLastMtl("Pr", 1)
    sc.addMaterial("metal")
    sc.setLastMtl("Pm", 1)
    sc.setLastMtl("Pr", 0.2)
    o = Obj()
    o.group("ground")
    o.quad((-6, 0, -2), (6, 0, -2), (6, 0, 10), (-6, 0, 10), (0, 1, 0))
    sc.addObjectText(o.text(), 0, parentDirectory="")
    sc.addEllipsoid((0.0, 0.5, 3.0), 1, 0, 0.5, 0)
    sc.addEllipsoid((1.1, 0.4, 2.5), 1, 0, 0.4, 1)
    sc.addEllipsoid((-1.0, 0.3, 2.2), (1.0, 2.0, 1.0), 0, 0.3, 0)
    return _finish("C1", sc, W, H, (0.0, 0.8, 0.0), (0.1, 0.0, 0.0), (153, 179, 230), sample_res, max_bounces)


def c2_cornell(W=1280, H=720, sample_res=8, max_bounces=8):
    """C2 diffuse-only Cornell box: 5 walls + light quad + 2 boxes = 36 triangles, black 1x1 sky."""
    sc = _new_scene()
    _cornell_materials(sc)
    o = Obj()
    _cornell_room(o)
    sc.addObjectText(o.text(), 0, parentDirectory="")
    return _finish("C2", sc, W, H, CORNELL_CAM, CORNELL_ROT, (0, 0, 0), sample_res, max_bounces)


def c3_glass_metal(W=1920, H=1080, sample_res=8, max_bounces=8, subdiv=3):
    """C3: Cornell room + glass and metal icospheres (1280 triangles each at subdiv 3, smooth vn)."""
    sc = _new_scene()
    _cornell_materials(sc)
    sc.addMaterial("glass")
    sc.setLastMtl("Tr", 0.9)
    sc.setLastMtl("Ni", 1.5)
    sc.setLastMtl("Pr", 1)
    sc.setLastMtl("Tf", (0.2, 0.05, 0.05))
    sc.setLastMtl("Density", 1)
    sc.addMaterial("metal")
    sc.setLastMtl("Pm", 1)
    sc.setLastMtl("Pr", 0.1)
    sc.setLastMtl("Kd", (0.9, 0.8, 0.5))
    o = Obj()
    _cornell_room(o, boxes=False)
    o.group("glass_sphere")
    o.usemtl("glass")
    o.mesh(*icosphere(subdiv, (-0.42, 0.45, -0.25), 0.45))
    o.group("metal_sphere")
    o.usemtl("metal")
    o.mesh(*icosphere(subdiv, (0.45, 0.5, 0.35), 0.5))
    sc.addObjectText(o.text(), 0, parentDirectory="")
    return _finish("C3", sc, W, H, CORNELL_CAM, CORNELL_ROT, (0, 0, 0), sample_res, max_bounces)


def c4_mesh(W=1920, H=1080, sample_res=8, max_bounces=8, nu=224, nv=224, seed=4):
    """C4: Cornell room + one seeded displaced-torus mesh of 2*nu*nv (= 100 352) triangles in ONE `o` group
    (one BVH, like the reference's single-object dragon, dispatch.java:257)."""
    sc = _new_scene()
    _cornell_materials(sc)
    sc.addMaterial("clay")
    sc.setLastMtl("Kd", (0.7, 0.55, 0.4))
    sc.setLastMtl("Pr", 1)
    o = Obj()
    _cornell_room(o, boxes=False)
    o.group("torus")
    o.usemtl("clay")
    v, n, f = displaced_torus(nu, nv, (0.0, 0.0, 0.0), 0.55, 0.22, 0.25, seed)
    # stand the torus up, tilted, in the middle of the room
    a, b = 1.0, 0.4
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    M = Ry @ Rx
    v = [tuple(M @ np.array(p) + np.array((0.0, 0.85, 0.1))) for p in v]
    n = [tuple(M @ np.array(q)) for q in n]
    o.mesh(v, n, f)
    sc.addObjectText(o.text(), 0, parentDirectory="")
    return _finish("C4", sc, W, H, CORNELL_CAM, CORNELL_ROT, (0, 0, 0), sample_res, max_bounces)


def c5_clearcoat_sss(W=3840, H=2160, sample_res=8, max_bounces=16, subdiv=4):
    """C5: Cornell room + clearcoat and subsurface meshes, plus the reference's "test" material (dispatch.java:228-239)."""
    sc = _new_scene()
    _cornell_materials(sc)
    sc.addMaterial("coat")
    sc.setLastMtl("Kd", (0.1, 0.2, 0.7))
    sc.setLastMtl("Ks", (0.9, 0.9, 0.9))
    sc.setLastMtl("Pc", 0.5)
    sc.setLastMtl("Pcr", 0.1)
    sc.setLastMtl("Pr", 1)
    sc.addMaterial("sss")
    sc.setLastMtl("Kd", (0.8, 0.45, 0.5))
    sc.setLastMtl("subsurface", 0.5)
    sc.setLastMtl("subsurfaceColor", (0.45, 0.8, 0.5))
    sc.setLastMtl("subsurfaceRadius", (1, 1, 1))
    sc.setLastMtl("Pr", 1)
    sc.addMaterial("test")                      # dispatch.java:228-239
    sc.setLastMtl("Kd", (0.8, 0.45, 0.5))
    sc.setLastMtl("Ks", (0.5, 0.5, 0.5))
    sc.setLastMtl("Ni", 1.45)
    sc.setLastMtl("Pr", 1)
    sc.setLastMtl("Pc", 0.0)
    sc.setLastMtl("Pcr", 0.0)
    sc.setLastMtl("Tr", 0.7)
    sc.setLastMtl("subsurface", 0)
    sc.setLastMtl("subsurfaceColor", (0.45, 0.8, 0.5))
    sc.setLastMtl("subsurfaceRadius", (1, 1, 1))
    sc.setLastMtl("Density", 0.1)
    o = Obj()
    _cornell_room(o, boxes=False)
    o.group("coat_sphere")
    o.usemtl("coat")
    o.mesh(*icosphere(subdiv, (0.45, 0.5, 0.3), 0.5))
    o.group("sss_sphere")
    o.usemtl("sss")
    o.mesh(*icosphere(subdiv, (-0.45, 0.4, -0.2), 0.4))
    o.group("test_sphere")
    o.usemtl("test")
    o.mesh(*icosphere(subdiv - 1, (0.0, 1.3, 0.0), 0.3))
    sc.addObjectText(o.text(), 0, parentDirectory="")
    return _finish("C5", sc, W, H, CORNELL_CAM, CORNELL_ROT, (0, 0, 0), sample_res, max_bounces)


def t1_textured(W=96, H=54, sample_res=8, max_bounces=8):
    """Texture-map workload (not a BASELINE config): Cornell room whose floor has a checker map_Kd, whose back
    wall carries map_Ke + map_Ks, a box with map_Pr / map_Pm / map_Pc / map_Tr, and a panel shaded through a raw-texel map_bump."""
    rs = np.random.RandomState(11)

    def tex(h, w, fn):
        a = np.zeros((h, w, 4), np.uint8)
        for j in range(h):
            for i in range(w):
                a[j, i, :3] = fn(i, j)
        a[..., 3] = 255
        return a

    textures = {
        1: tex(8, 8, lambda i, j: (230, 230, 230) if (i + j) % 2 else (40, 60, 200)),                      # checker albedo
        2: tex(4, 16, lambda i, j: (255, 200, 120) if i % 4 == 0 else (0, 0, 0)),                           # emissive stripes
        3: tex(5, 7, lambda i, j: tuple(int(v) for v in rs.randint(0, 256, 3))),                              # noise (Ks / Pr / Pm / Pc / Tr source)
        4: tex(2, 2, lambda i, j: (60, 230, 90)),                                                             # "normal" texels, used raw (frag.glsl:827)
    }
    sc = _new_scene()
    _cornell_materials(sc)
    sc.addMaterial("floor"); sc.setLastMtl("Kd", (0.9, 0.9, 0.9)); sc.setLastMtl("Pr", 1); sc.setLastMtl("map_Kd", 1)
    sc.addMaterial("glow"); sc.setLastMtl("Kd", (0.5, 0.5, 0.5)); sc.setLastMtl("Pr", 1); sc.setLastMtl("map_Ke", 2); sc.setLastMtl("map_Ks", 3); sc.setLastMtl("Pc", 0.3)
    sc.addMaterial("mixed"); sc.setLastMtl("Kd", (0.8, 0.7, 0.6)); sc.setLastMtl("map_Pr", 3); sc.setLastMtl("map_Pm", 3); sc.setLastMtl("map_Pc", 3)
    sc.setLastMtl("map_Tr", 3); sc.setLastMtl("Ni", 1.3); sc.setLastMtl("map_Ka", 1); sc.setLastMtl("Ka", (0.1, 0.1, 0.1))
    sc.addMaterial("bumped"); sc.setLastMtl("Kd", (0.7, 0.7, 0.7)); sc.setLastMtl("Pr", 1); sc.setLastMtl("map_bump", 4)
    o = Obj()
    o.group("room")
    o.usemtl("floor")
    o.quad_uv((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, 1, 0), (0.05, 0.05), (3.95, 3.95))
    o.usemtl("white")
    o.quad((-1, 2, -1), (-1, 2, 1), (1, 2, 1), (1, 2, -1), (0, -1, 0))
    o.usemtl("glow")
    o.quad_uv((-1, 0, 1), (1, 0, 1), (1, 2, 1), (-1, 2, 1), (0, 0, -1))
    o.usemtl("red")
    o.quad((1, 0, -1), (1, 2, -1), (1, 2, 1), (1, 0, 1), (-1, 0, 0))
    o.usemtl("green")
    o.quad((-1, 0, -1), (-1, 0, 1), (-1, 2, 1), (-1, 2, -1), (1, 0, 0))
    o.group("light")
    o.usemtl("light")
    o.quad((-0.25, 1.98, -0.25), (0.25, 1.98, -0.25), (0.25, 1.98, 0.25), (-0.25, 1.98, 0.25), (0, -1, 0))
    o.group("panel")
    o.usemtl("bumped")
    o.quad_uv((-0.9, 0.2, 0.2), (-0.3, 0.2, -0.4), (-0.3, 1.2, -0.4), (-0.9, 1.2, 0.2), (0.7, 0.1, -0.7))
    o.usemtl("mixed")
    o.quad_uv((0.2, 0.1, 0.3), (0.9, 0.1, -0.2), (0.9, 1.0, -0.2), (0.2, 1.0, 0.3), (-0.58, 0.05, -0.81))
    sc.addObjectText(o.text(), 0, parentDirectory="")
    wl = _finish("T1", sc, W, H, CORNELL_CAM, CORNELL_ROT, (30, 40, 60), sample_res, max_bounces)
    wl.textures = textures
    return wl


def m1_moving(step=0, W=96, H=54, sample_res=8, max_bounces=8, subdiv=2, textured=True, light_dx=0.0):
    """M1, the moving-geometry workload of include/pt_motion.h (not a BASELINE config): the Cornell room without its boxes plus four things whose
    pose is a function of `step` — a box that translates and turns about y, a smooth-normal icosphere that rotates about its centre, a textured
    quad that translates, an ellipsoid that translates and grows.  Everything is built in the same order at every step, so triangle k and
    ellipsoid k are the same piece of surface throughout; step 0 is the rest pose.  Every material is diffuse; textured=False leaves the quad's
    map_Kd out (the same triangles, no texture table).  light_dx slides the light quad along x (m2_relit)."""
    s = float(step)
    sc = _new_scene()
    _cornell_materials(sc)
    sc.addMaterial("poster"); sc.setLastMtl("Kd", (0.9, 0.9, 0.9)); sc.setLastMtl("Pr", 1)
    if textured:
        sc.setLastMtl("map_Kd", 1)
    ball = sc.addMaterial("ball"); sc.setLastMtl("Kd", (0.2, 0.3, 0.7)); sc.setLastMtl("Pr", 1)
    o = Obj()
    _cornell_room(o, boxes=False, light_dx=light_dx)
    o.group("box")
    o.usemtl("white")
    o.box((0.45 + 0.02 * s, 0.3, 0.15 - 0.01 * s), (0.25, 0.3, 0.25), 0.3 + 0.02 * s)
    o.group("sphere")
    o.usemtl("green")
    c = np.array((-0.45, 0.4, 0.25))
    verts, normals, faces = icosphere(subdiv, (0.0, 0.0, 0.0), 0.35)
    a = 0.02 * s
    R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    o.mesh([tuple(c + R @ np.array(p)) for p in verts], [tuple(R @ np.array(n)) for n in normals], faces)
    o.group("poster")
    o.usemtl("poster")
    dx = 0.015 * s
    o.quad_uv((0.3 + dx, 0.9, 0.6), (-0.3 + dx, 0.9, 0.6), (-0.3 + dx, 1.5, 0.6), (0.3 + dx, 1.5, 0.6), (0, 0, -1))
    sc.addObjectText(o.text(), 0, parentDirectory="")
    sc.addEllipsoid((0.0 + 0.01 * s, 0.25 + 0.005 * s, -0.45), 1, 0, 0.2 + 0.005 * s, ball)
    wl = _finish("M1", sc, W, H, CORNELL_CAM, CORNELL_ROT, (0, 0, 0), sample_res, max_bounces)
    tex = np.zeros((8, 8, 4), np.uint8)
    for j in range(8):
        for i in range(8):
            tex[j, i, :3] = (230, 200, 60) if (i + j) % 2 else (60, 40, 160)
    tex[..., 3] = 255
    wl.textures = {1: tex} if textured else {}
    return wl


def m1_refit(step=0, W=96, H=54, **kw):
    """M1 at `step` over the rest pose's trees, the input of a BVH refit (include/pt_refit.h): bindings 3 and 7 (and everything else) of
    m1_moving(step), bindings 10-13 of m1_moving(0).  Binding 10 is the REST pose's and stale for step != 0: the caller fills it in with its plan,
    `wl.buffers[10], cost = renderer.RefitPlan(wl.buffers).run(wl.buffers[3])`."""
    rest, wl = m1_moving(0, W, H, **kw), m1_moving(step, W, H, **kw)
    assert rest.buffers[3].size == wl.buffers[3].size
    b = dict(wl.buffers)
    for k in (10, 11, 12, 13):
        b[k] = rest.buffers[k].copy()
    return Workload("M1", W, H, b, wl.sky, wl.sample_res, wl.max_bounces, dict(rest.info), wl.textures)


def m2_relit(step=0, W=96, H=54, **kw):
    """M2, the relit workload of include/pt_validate.h (not a BASELINE config): M1's rest pose with the light quad slid by 0.05 * step along x.
    No surface but the light moves; the shadows and the lit walls change everywhere else."""
    wl = m1_moving(0, W, H, light_dx=0.05 * float(step), **kw)
    wl.name = "M2"
    return wl


def m3_tube(W=96, H=54, sample_res=8, max_bounces=8, n_seg=12, n_around=10):
    """M3's rest pose, the skinning workload of include/pt_skin.h (not a BASELINE config): M1's room without M1's movers plus an upright tube
    with smooth normals, n_seg rings of 2 * n_around triangles along its axis (+y) and a disc that closes its lower end.  The tube's triangles
    are the last ones of binding 3 (the room's come first), the disc's n_around the very last: info["tube"] = (first, n_side, n_cap) and
    info["axis"] = (cx, y0, y1, cz) say where."""
    sc = _new_scene()
    _cornell_materials(sc)
    o = Obj()
    _cornell_room(o, boxes=False)
    o.group("tube")
    o.usemtl("green")
    cx, cz, y0, y1, rad = 0.1, 0.2, 0.05, 1.45, 0.12
    verts, normals, faces = [], [], []
    for i in range(n_seg + 1):
        y = y0 + (y1 - y0) * i / n_seg
        for j in range(n_around):
            u = 2 * math.pi * (j + 0.37) / n_around              # (no normal with an exactly-zero component: SURVEY.md Q-4)
            verts.append((cx + rad * math.cos(u), y, cz + rad * math.sin(u)))
            normals.append((math.cos(u), 0.0123, math.sin(u)))
    for i in range(n_seg):
        for j in range(n_around):
            a, b = i * n_around + j, i * n_around + (j + 1) % n_around
            c, d = b + n_around, a + n_around
            faces += [(a, c, b), (a, d, c)]
    first_v = o.nv
    o.mesh(verts, normals, faces)
    centre, down = o.v((cx, y0, cz)), o.vn((0.0, -1.0, 0.0))
    for j in range(n_around):
        o.f(centre, first_v + 1 + j, first_v + 1 + (j + 1) % n_around, down)
    sc.addObjectText(o.text(), 0, parentDirectory="")
    wl = _finish("M3", sc, W, H, CORNELL_CAM, CORNELL_ROT, (0, 0, 0), sample_res, max_bounces)
    n_side = 2 * n_seg * n_around
    wl.info["tube"] = (wl.buffers[3].size // 40 - n_side - n_around, n_side, n_around)
    wl.info["axis"] = (cx, y0, y1, cz)
    return wl


def ramp_weights(t, n_bones):
    """The two tables of include/pt_skin.h for corners at parameter t in [0, 1] along a chain of n_bones joints (t < 0: a static corner): a
    linear ramp between the two nearest joints, one slot where the ramp is 0 or 1.  t: any shape -> (bone, weight) of shape t.shape + (4,)."""
    t = np.asarray(t, np.float64)
    bone = np.full(t.shape + (4,), -1, np.int32)
    weight = np.zeros(t.shape + (4,), np.float32)
    s = np.round(np.clip(t, 0.0, 1.0) * (n_bones - 1) * 4096.0) / 4096.0      # (in steps of 1/4096: a corner at a joint's height has one slot)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_bones - 1)
    f = (s - i0).astype(np.float32)
    used, two = t >= 0.0, (t >= 0.0) & (f > 0.0)
    bone[..., 0] = np.where(used, i0, -1)
    weight[..., 0] = np.where(two, np.float32(1.0) - f, np.where(used, 1.0, 0.0))
    bone[..., 1] = np.where(two, i0 + 1, -1)
    weight[..., 1] = np.where(two, f, 0.0)
    return bone, weight


def chain_records(n_bones, pivots, axis, angle):
    """n_bones records of 24 floats (include/pt_pose.h): joint i turned by i * angle about `axis`, each joint hinged at pivots[i] on the joint
    below it, so the chain stays connected.  Binary64, rounded once; N is the rotation itself."""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R1 = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)
    out = np.zeros((n_bones, 24), np.float32)
    A, t = np.eye(3), np.zeros(3)                                  # joint i - 1: x -> A x + t
    for i in range(n_bones):
        if i:
            p = np.asarray(pivots[i], np.float64)
            A, t = A @ R1, A @ (p - R1 @ p) + t                  # first the hinge at p, then the joints below
        out[i, :12] = np.concatenate([A, t.reshape(3, 1)], axis=1).reshape(12)
        out[i, 12:21] = A.reshape(9)
    return out


def m3_bending(step=0, W=96, H=54, n_bones=5, a=0.04, **kw):
    """M3 at `step`: (the rest pose's workload, corner_bone, corner_weight, the records).  The tables (12 words per triangle) weight each corner
    of the tube's side between its two nearest joints by its height; the disc and the room are static.  Joint i is turned by i * step * a about
    +z.  Two corners at one rest vertex get the same words, so the posed tube has no cracks."""
    wl = m3_tube(W, H, **kw)
    first, n_side, _ = wl.info["tube"]
    cx, y0, y1, cz = wl.info["axis"]
    tris = wl.buffers[3].reshape(-1, 40)
    t = np.full((tris.shape[0], 3), -1.0)
    y = tris[first:first + n_side, 1:12:4].astype(np.float64)       # the three vertices' y
    t[first:first + n_side] = np.clip((y - y0) / (y1 - y0), 0.0, 1.0)
    bone, weight = ramp_weights(t, n_bones)
    return wl, bone.reshape(-1), weight.reshape(-1), m3_records(wl, step, n_bones, a)


def m3_records(wl, step, n_bones=5, a=0.04):
    """the records of m3_bending(step) alone, for a workload of m3_tube: the hinge of joint i lies on the axis half way between joints i - 1 and i"""
    cx, y0, y1, cz = wl.info["axis"]
    pivots = [(cx, y0 + (y1 - y0) * max(i - 0.5, 0.0) / (n_bones - 1), cz) for i in range(n_bones)]
    return chain_records(n_bones, pivots, (0.0, 0.0, 1.0), float(step) * a)


def ring_bulges(tris, moving, heights, width, amp):
    """Morph targets of include/pt_morph.h for the corners `moving` (3 * k + c) of binding 3: target t is a ring-shaped bulge at height
    heights[t] (+y), a Gaussian profile of the given width.  The vertex delta runs along the corner's rest normal with the profile's amplitude;
    the normal delta tilts the normal against the profile's slope.  Both are functions of the corner's own rest floats, computed in binary64
    and rounded once, so corners that share a vertex get identical entries.  -> a list of (corners int32[m], deltas float32[m, 6])"""
    tris = np.asarray(tris, np.float32).reshape(-1, 40)
    q = np.asarray(moving, np.int64).reshape(-1)
    k, c = q // 3, q % 3
    v = np.stack([tris[k, 4 * c + j] for j in range(3)], axis=1).astype(np.float64)
    n = np.stack([tris[k, 12 + 4 * c + j] for j in range(3)], axis=1).astype(np.float64)
    out = []
    for h in heights:
        u = (v[:, 1] - h) / width
        g = amp * np.exp(-u * u)
        named = g > 0.01 * amp
        slope = -2.0 * u * g / width                              # d(profile) / dy
        d = np.zeros((q.size, 6))
        d[:, :3] = g[:, None] * n
        d[:, 4] = -slope                                          # first order: the normal leans away from the rising side
        out.append((q[named].astype(np.int32), d[named].astype(np.float32)))
    return out


def m4_weights(step, n_targets=3):
    """the morph weights of m4_bulging(step): target t swells and shrinks at its own pace; step 0 is the unmorphed pose"""
    return np.abs(np.sin(0.4 * float(step) * (np.arange(n_targets) + 1.0))).astype(np.float32)


def m4_bulging(step=0, W=96, H=54, n_bones=5, a=0.04, n_targets=3, **kw):
    """M4 at `step`, the morph workload of include/pt_morph.h (not a BASELINE config): M3's tube and skin plus n_targets ring-shaped bulges at
    evenly spaced heights of the tube's side.  -> (the rest pose's workload, corner_bone, corner_weight, the targets, the records, the morph
    weights); only the last two depend on step."""
    wl, bone, weight, X = m3_bending(step, W, H, n_bones, a, **kw)
    wl.name = "M4"
    first, n_side, _ = wl.info["tube"]
    cx, y0, y1, cz = wl.info["axis"]
    moving = np.arange(3 * first, 3 * (first + n_side))
    heights = [y0 + (y1 - y0) * (t + 1.0) / (n_targets + 1.0) for t in range(n_targets)]
    targets = ring_bulges(wl.buffers[3], moving, heights, 0.12 * (y1 - y0), 0.05)
    return wl, bone, weight, targets, X, m4_weights(step, n_targets)


def weld_corners(tris, moved, keep_creases=True):
    """The vertex ids of include/pt_normals.h for binding 3 (40 floats per triangle): the corners `moved` (3 * k + c, those the pose's rule moves)
    with a bitwise-equal rest position are one vertex; with keep_creases they must have a bitwise-equal rest normal as well, so a hard edge
    stays hard.  Ids are dense and ascend with the first corner that names them.  All other corners get -1, and so does a corner whose vertex an
    earlier corner of its own triangle names already (a degenerate triangle: an id may stand once per triangle).
    -> (corner_vertex int32[3 * n_tris], n_vertices)"""
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 40).view(np.uint32)
    q = np.unique(np.asarray(moved, np.int64).reshape(-1))
    ids = np.full(3 * t.shape[0], -1, np.int32)
    if q.size == 0:
        return ids, 0
    k, c = q // 3, q % 3
    cols = [4 * c + j for j in range(3)] + ([12 + 4 * c + j for j in range(3)] if keep_creases else [])
    key = np.stack([t[k, col] for col in cols], axis=1)
    _, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(np.argsort(first))                            # dense ids in the order of each vertex's first corner
    g = order[inverse].astype(np.int32)
    # once per triangle: q ascends, so a triangle's corners are neighbours
    same1 = (k[1:] == k[:-1]) & (g[1:] == g[:-1])
    same2 = (k[2:] == k[:-2]) & (g[2:] == g[:-2])
    g[1:][same1] = -1
    g[2:][same2] = -1
    ids[q] = g
    used = np.unique(g[g >= 0])
    if used.size != int(first.size):                                 # an id that only dropped corners named: renumber densely
        remap = np.full(int(first.size), -1, np.int32); remap[used] = np.arange(used.size, dtype=np.int32)
        ids[ids >= 0] = remap[ids[ids >= 0]]
    return ids, int(used.size)


def m5_rippling(step=0, W=96, H=54, **kw):
    """M5 at `step`, the workload of include/pt_normals.h (not a BASELINE config): M4's tube, skin and targets plus the welded vertex ids of the
    tube's side, from which its normals are recomputed after every step.  -> what m4_bulging returns, then corner_vertex and n_vertices."""
    wl, bone, weight, targets, X, w = m4_bulging(step, W, H, **kw)
    wl.name = "M5"
    first, n_side, _ = wl.info["tube"]
    ids, n_vertices = weld_corners(wl.buffers[3], np.arange(3 * first, 3 * (first + n_side)), keep_creases=True)
    return wl, bone, weight, targets, X, w, ids, n_vertices


def m6_records(wl, step, n_bones=5, a=0.25):
    """the records of m6_twisting(step) alone, for a workload of m3_tube: joint i turned by i * step * a about +y, the tube's axis, on which the
    pivots lie (so the records are pure rotations about that axis: the chain twists and nothing bends)"""
    cx, y0, y1, cz = wl.info["axis"]
    pivots = [(cx, y0 + (y1 - y0) * max(i - 0.5, 0.0) / (n_bones - 1), cz) for i in range(n_bones)]
    return chain_records(n_bones, pivots, (0.0, 1.0, 0.0), float(step) * a)


def m6_twisting(step=0, W=96, H=54, n_bones=5, a=0.25, **kw):
    """M6 at `step`, the workload of include/pt_skin_dq.h (not a BASELINE config): M3's tube and ramp weights, twisted instead of bent.  Between
    two joints twisted against each other the linear skin of include/pt_skin.h pulls the tube's wall towards its axis; the dual-quaternion skin
    keeps its radius.  -> what m3_bending returns: (the rest pose's workload, corner_bone, corner_weight, the records)."""
    wl, bone, weight, _ = m3_bending(0, W, H, n_bones, **kw)
    wl.name = "M6"
    return wl, bone, weight, m6_records(wl, step, n_bones, a)


def m7_rig(wl, n_bones=5, a=0.16, times=(0.0, 1.0, 2.5), bends=(0.0, 1.0, -0.5)):
    """The rig of m7_chained for a workload of m3_tube, in the terms of include/pt_rig.h: (parent int32[n_bones], inv_bind float32[n_bones, 12],
    times float32[n_keys], values float32[n_keys, n_bones, 12]).  Joint i is the child of joint i - 1 and sits at M3's hinge i on the tube's
    axis: its local translation is the step from the hinge below, its inverse bind the shift of its hinge to the origin.  In key k every joint
    but the root turns locally by bends[k] * a about +z, so the bend accumulates down the chain: joint i's record is the turn by
    i * bends[k] * a that m3_records makes, up to rounding.  Binary64, rounded once."""
    cx, y0, y1, cz = wl.info["axis"]
    pivots = np.array([(cx, y0 + (y1 - y0) * max(i - 0.5, 0.0) / (n_bones - 1), cz) for i in range(n_bones)])
    parent = np.arange(-1, n_bones - 1, dtype=np.int32)
    inv_bind = np.zeros((n_bones, 3, 4))
    inv_bind[:, :, :3] = np.eye(3)
    inv_bind[:, :, 3] = -pivots
    values = np.zeros((len(times), n_bones, 12))
    values[:, :, 8:11] = 1.0
    values[:, 0, 0:3] = pivots[0]
    values[:, 1:, 0:3] = pivots[1:] - pivots[:-1]
    values[:, :, 7] = 1.0
    for k, bend in enumerate(bends):
        half = 0.5 * float(bend) * a
        values[k, 1:, 6], values[k, 1:, 7] = math.sin(half), math.cos(half)      # (x y z w) of a turn about +z
    return parent, inv_bind.reshape(n_bones, 12).astype(np.float32), np.asarray(times, np.float32), values.astype(np.float32)


def m7_chained(W=96, H=54, n_bones=5, a=0.16, **kw):
    """M7, the workload of include/pt_rig.h (not a BASELINE config): M3's tube and ramp weights with its joints as one chain, animated by a
    clip of three keys instead of by records.  -> (the rest pose's workload, corner_bone, corner_weight, parent, inv_bind, times, values);
    the last four are m7_rig's."""
    wl, bone, weight, _ = m3_bending(0, W, H, n_bones, **kw)
    wl.name = "M7"
    return (wl, bone, weight) + m7_rig(wl, n_bones, a)


def m8_rig(wl, n_bones=5, a=0.16, b=0.25):
    """The rig of m8_mixed for a workload of m3_tube, in the terms of include/pt_rig_mix.h: (parent, inv_bind, clips, mask).  parent and
    inv_bind are m7_rig's.  clips[0] is m7_rig's bend about +z; clips[1] has its own key times and twists every joint but the root locally by
    twists[k] * b about +y, the tube's axis, as m6_records does.  Each is (times float32[n_keys], values float32[n_keys, n_bones, 12]); key 0 of
    both is the rest pose.  mask float32[n_bones] ramps from 0 at the root to 1 at the tip."""
    parent, inv_bind, times, bend = m7_rig(wl, n_bones, a)
    _, _, times2, twist = m7_rig(wl, n_bones, b, times=(0.0, 0.75, 2.0, 3.0), bends=(0.0, 1.0, -1.0, 0.5))
    twist[:, :, 5], twist[:, :, 6] = twist[:, :, 6].copy(), 0.0        # (x y z w): the turn about +z becomes the same turn about +y
    mask = (np.arange(n_bones) / max(n_bones - 1, 1)).astype(np.float32)
    return parent, inv_bind, [(times, bend), (times2, twist)], mask


def m8_layers(step):
    """the layers of m8_mixed at `step`, as renderer.rig_layers takes them: the bend looping as the base, the twist looping at its own pace
    faded in and out over it, and the bend once more, slower, added through the mask (slot 0)"""
    s = float(step)
    fade = 0.5 - 0.5 * math.cos(0.2 * s)
    return [dict(clip=0, t=0.3 * s, wrap="loop"),
            dict(clip=1, t=0.4 * s, weight=fade, wrap="loop"),
            dict(clip=0, t=0.45 * s, weight=0.75, mask=0, mode="additive", wrap="loop")]


def m8_mixed(step=0, W=96, H=54, n_bones=5, **kw):
    """M8 at `step`, the workload of include/pt_rig_mix.h (not a BASELINE config): M7's chain with two clips in slots, M7's bend and a twist
    about the tube's axis, and a mask that ramps from the root to the tip.  -> (the rest pose's workload, corner_bone, corner_weight, parent,
    inv_bind, clips, mask, layers); only the layers depend on step (m8_layers), the four before them are m8_rig's."""
    wl, bone, weight, _ = m3_bending(0, W, H, n_bones, **kw)
    wl.name = "M8"
    return (wl, bone, weight) + m8_rig(wl, n_bones) + (m8_layers(step),)


M9_CONSTRAINTS = [dict(kind="two_bone", joint=4, pole=True)]            # joints 2-3-4 of the chain: root 2, mid 3, tip 4


def m9_goals(wl, step, n_bones=5):
    """the goals of m9_reaching at `step`, as renderer.rig_ik_goals takes them: the target circles beside the tube at the height of the chain's
    mid, within the two bones' reach of the chain's root; the pole stands off to the side the target circles on, so the chain bends outwards"""
    cx, y0, y1, cz = wl.info["axis"]
    bone = (y1 - y0) / (n_bones - 1)
    s = 0.35 * float(step)
    root_y = y0 + 1.5 * bone                                           # hinge 2
    target = (cx + 0.9 * bone * math.cos(s), root_y + bone, cz + 0.9 * bone * math.sin(s))
    pole = (cx + 4.0 * bone * math.cos(s + 0.6), root_y + 0.5 * bone, cz + 4.0 * bone * math.sin(s + 0.6))
    return [dict(target=target, weight=1.0, pole=pole)]


def m9_reaching(step=0, W=96, H=54, n_bones=5, **kw):
    """M9 at `step`, the workload of include/pt_rig_ik.h (not a BASELINE config): M8's tube, clips, mask and layers, with joints 2-3-4 as a
    two-bone chain whose tip follows a target circling beside the tube, bent towards a pole.  -> what m8_mixed returns, then the constraints
    (M9_CONSTRAINTS) and the goals of the step (m9_goals)."""
    out = m8_mixed(step, W, H, n_bones, **kw)
    out[0].name = "M9"
    return out + (list(M9_CONSTRAINTS), m9_goals(out[0], step, n_bones))


def asset_workload(directory, W, H, cam=CORNELL_CAM, rot=CORNELL_ROT, sky=(30, 40, 60), sample_res=8, max_bounces=8, name="asset",
                   scale=1.0, shift=0.0, rotate=0.0, **pk):
    """The reference's way of loading a model (dispatch.java:219-229 + :869-882): texture 0 is the sky, then
    scene.addObject(<directory>) parses every .mtl (registering the map files) and every .obj in it; the decoded images fill
    the rest of the texture table.  `sky` is an RGB triple or a path to an image."""
    sc = _new_scene()
    sky_img = sky
    if isinstance(sky, str):
        from PIL import Image
        sc.addTexture(sky, "skybox.png")
        sky_img = np.asarray(Image.open(sky).convert("RGBA"), dtype=np.uint8).copy()
    else:
        sc.addTexture("", "skybox.png")
    sc.addMaterial("default")
    sc.addObject(directory, 0, scale, shift, rotate)
    wl = _finish(name, sc, W, H, cam, rot, sky_img, sample_res, max_bounces, **pk)
    wl.textures = {i: a for i, a in sc.load_textures().items() if i >= 1}
    return wl


def c6_many_objects(W=1920, H=1080, sample_res=8, max_bounces=8, groups=64, nu=28, nv=28, seed=6):
    """C6: the shape of the scenes the reference's author lists (dispatch.java:245-264: multi-group OBJs with dozens of `o` groups — one BVH
    each, frag.glsl:563-577 loops over all of them — next to addEllipsoid calls): the Cornell room's two groups + (groups - 2) seeded
    displaced tori of 2*nu*nv triangles each in a 4x4x4 lattice (64 groups: 97 228 triangles), materials cycling through diffuse / metal /
    glass / clearcoat, plus 3 ellipsoids (one stretched, one rotated)."""
    sc = _new_scene()
    _cornell_materials(sc)
    names = []
    for k, (kd, extra) in enumerate([((0.7, 0.55, 0.4), {}), ((0.9, 0.8, 0.5), dict(Pm=1, Pr=0.1)), ((0.9, 0.9, 0.9), dict(Tr=0.9, Ni=1.5, Tf=(0.05, 0.2, 0.05), Density=1)),
                                     ((0.1, 0.2, 0.7), dict(Ks=(0.9, 0.9, 0.9), Pc=0.5, Pcr=0.1)), ((0.3, 0.6, 0.35), {}), ((0.6, 0.3, 0.6), dict(Pm=0.5, Pr=0.4))]):
        names.append(f"m{k}")
        sc.addMaterial(names[-1])
        sc.setLastMtl("Kd", kd)
        sc.setLastMtl("Pr", 1)
        for key, val in extra.items():
            sc.setLastMtl(key, val)
    o = Obj()
    _cornell_room(o, boxes=False)
    rs = np.random.RandomState(seed)
    cells = [(i, j, k) for k in range(4) for j in range(4) for i in range(4)]
    for g in range(groups - 2):
        i, j, k = cells[g % len(cells)]
        centre = np.array((-0.75 + 0.5 * i, 0.25 + 0.48 * j, -0.75 + 0.5 * k)) + rs.uniform(-0.04, 0.04, size=3)
        v, n, f = displaced_torus(nu, nv, (0.0, 0.0, 0.0), 0.13, 0.055, 0.25, seed * 1000 + g)
        a, b = rs.uniform(0, math.pi, size=2)
        Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
        Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
        M = Ry @ Rx
        o.group(f"torus{g}")
        o.usemtl(names[g % len(names)])
        o.mesh([tuple(M @ np.array(p) + centre) for p in v], [tuple(M @ np.array(q)) for q in n], f)
    sc.addObjectText(o.text(), 0, parentDirectory="")
    sc.addEllipsoid((0.0, 1.0, 0.0), 1, 0, 0.16, 5)
    sc.addEllipsoid((0.5, 0.75, -0.5), (1.0, 2.5, 1.0), 0, 0.12, 4)
    sc.addEllipsoid((-0.5, 1.25, 0.5), (2.0, 1.0, 1.0), (0.3, 0.2, 0.1), 0.14, 7)
    return _finish("C6", sc, W, H, CORNELL_CAM, CORNELL_ROT, (0, 0, 0), sample_res, max_bounces)


def equirect_sky(h, w, seed=9):
    """A synthetic equirect sky image (h, w, 4) uint8 in place of the reference's thatch_chapel_4k.png (dispatch.java:221, not in the repository): smooth
    gradients + seeded noise + a small "sun", every texel different from its neighbours, so that the bilinear REPEAT sampler (frag.glsl:235-242) is
    exercised on every miss."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, 4), np.float64)
    img[..., 0] = 90 + 80 * np.sin(2 * np.pi * x / w) + 40 * y / h
    img[..., 1] = 110 + 60 * np.cos(4 * np.pi * x / w) * (1 - y / h)
    img[..., 2] = 200 - 120 * y / h
    img[..., :3] += rs.uniform(-12, 12, size=(h, w, 3))
    sun = (x - 0.3 * w) ** 2 + (y - 0.25 * h) ** 2 < (0.02 * w) ** 2
    img[sun, :3] = 255
    img[..., 3] = 255
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


BUILDERS = {"C1": c1_spheres, "C2": c2_cornell, "C3": c3_glass_metal, "C4": c4_mesh, "C5": c5_clearcoat_sss, "C6": c6_many_objects}


def build(name, W=None, H=None, **kw):
    if name == "T1":
        return t1_textured(W or 96, H or 54, **kw)
    if name == "M1":
        return m1_moving(kw.pop("step", 0), W or 96, H or 54, **kw)
    if name == "M2":
        return m2_relit(kw.pop("step", 0), W or 96, H or 54, **kw)
    if name == "M3":
        return m3_tube(W or 96, H or 54, **kw)
    if name == "M4":
        return m4_bulging(kw.pop("step", 0), W or 96, H or 54, **kw)[0]
    if name == "M5":
        return m5_rippling(kw.pop("step", 0), W or 96, H or 54, **kw)[0]
    cfg = CONFIGS[name]
    W = cfg["W"] if W is None else W
    H = cfg["H"] if H is None else H
    kw.setdefault("sample_res", cfg["sample_res"])
    kw.setdefault("max_bounces", cfg["bounces"])
    return BUILDERS[name](W, H, **kw)
