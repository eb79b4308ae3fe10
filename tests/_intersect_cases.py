"""The scenes, ray sets and comparisons the tests of tests/_intersect_ref64.py share (tests/test_intersect_ref64.py on the CPU,
tests/test_gpu_intersect_ref64.py on the GPU).  Scenes are built once per process; nothing here is changed after it is made.

Which triangles are in a scene.  Binding 3 may hold triangles that no leaf range names (the loose triangles of addTri, the triangle an empty leaf
used to hold): the shader never tests them.  in_scene() hands the reference a binding 3 in which those triangles have three equal vertices —
e1 = e2 = 0, det = 0 in every arithmetic — and the ids of the others unchanged.  It reads the leaf ranges and binding 12; it reads no box."""
import copy

import numpy as np

import _intersect_ref64 as R64
import _move_cases as MC
import _normals_model as NM
import _refit_cases as RC
import _refit_model as RM

f32 = np.float32
N_RAYS = 4096
MOVED = ["soup2", "soup65", "soup257", "soup1000", "objects70", "ladder60", "emptyleaf", "leafroot"]
STATIC = {"C1": ("C1", {}), "C1rot": ("C1", {}), "C2": ("C2", {}), "C3": ("C3", {}), "C5": ("C5", dict(subdiv=2)),
          "C6": ("C6", dict(groups=24, nu=6, nv=6)), "C6g70": ("C6", dict(groups=70, nu=4, nv=4))}
SETS = ["random", "interior", "edges", "vertices"]
# |t - t_ref|, |u - u_ref| and |v - v_ref| <= BOUND_K * unit(), unit() = 2^-24 (|o|_inf + |t| + extent) / |n . d|: four times the largest
# multiple measured for the oracle over every scene and ray set of tests/test_intersect_ref64.py (MEASURED_K there)
MEASURED_K = 203.6
BOUND_K = 4.0 * MEASURED_K
_CACHE = {}


class Case:
    """a complete scene: buffers (every binding), tex ({index: texture}, 0 the sky), size (W, H)"""

    def __init__(self, name, buffers, tex, size):
        self.name, self.buffers, self.tex, self.size = name, buffers, tex, size


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


_PINNED = {}


def _id(a):
    """id(a) as a cache key: the array is kept, so the id is never handed out again"""
    _PINNED[id(a)] = a
    return id(a)


def c1rot(wl):
    """test_gpu_parity's C1rot: C1 with its three ellipsoids rotated and stretched"""
    b = dict(wl.buffers); e = b[7].copy(); ne = int(e[0])
    e[1 + 6 * ne: 1 + 9 * ne] = [0.3, 0.2, 0.1, -0.4, 0.0, 0.25, 0.0, 1.1, 0.0]
    e[1 + 3 * ne: 1 + 6 * ne] = [1.0, 2.0, 0.5, 1.5, 1.0, 1.0, 0.7, 0.7, 2.0]
    b[7] = e
    wl = copy.copy(wl); wl.buffers = b
    return wl


def static(pt, name):
    def make():
        base, kw = STATIC[name]
        wl = pt.scenes.build(base, 96, 54, **kw)
        if name == "C1rot":
            wl = c1rot(wl)
        b, tex = MC.workload_inputs(wl)
        return Case(name, b, tex, (wl.W, wl.H))
    return _once(("static", name), make)


def moved(pt, name, seed=7):
    """(the scene before the move, the scene after it: binding 3 perturbed, binding 10 the refit model's)"""
    def make():
        old = MC.scenes(pt)[name]
        tris, data = MC.moved(pt, name, seed) if seed == 7 else MC.move_of(old, RC.perturbed(old[3], seed))
        new = dict(old); new[3] = tris; new[10] = data
        return Case(name, old, MC.SKY, (MC.W, MC.H)), Case(f"{name}+{seed}", new, MC.SKY, (MC.W, MC.H))
    return _once(("moved", name, seed), make)


def m1(pt, step=4):
    """(M1's rest pose, M1 at `step` over the rest pose's topology)"""
    def make():
        rest = pt.scenes.m1_moving(0)
        wl = pt.scenes.m1_refit(step)
        wl.buffers[10] = RM.refit_buffers(wl.buffers)[0]
        old, tex = MC.workload_inputs(rest)
        return Case("M1", old, tex, (rest.W, rest.H)), Case(f"M1@{step}", dict(wl.buffers), tex, (rest.W, rest.H))
    return _once(("M1", step), make)


def m5(pt, step):
    """(M5's rest pose, M5 at `step` by the models: the morphed, skinned and re-smoothed triangles over the rest pose's refit tree)"""
    def make():
        rest, bone, weight, targets, X, w, ids, nv = pt.scenes.m5_rippling(step)
        old, tex = MC.workload_inputs(rest)
        new = dict(old)
        new[3], new[10] = MC.move_of(old, NM.morph_skin_smooth(old[3], targets, w, bone, weight, X, ids))
        return Case("M5", old, tex, (rest.W, rest.H)), Case(f"M5@{step}", new, tex, (rest.W, rest.H))
    return _once(("M5", step), make)


def refit_onto(old, tris):
    """the buffers of `old` with binding 3 = tris and the binding 10 the refit model gives it"""
    new = dict(old)
    new[3], new[10] = MC.move_of(old, tris)
    return new


def referenced(b):
    """bool per triangle of binding 3: named by the range of a leaf some root of binding 13 reaches"""
    n_tri = np.asarray(b[3]).size // 40
    seen = np.zeros(n_tri, bool)
    tree = np.asarray(b[11], np.int32).reshape(-1, 3)
    data = np.asarray(b[10], f32).reshape(-1, 8)
    leaf = np.asarray(b[12], np.int32)
    stack = [int(r) for r in np.asarray(b[13], np.int32)[1:1 + int(b[13][0])]]
    while stack:
        k = stack.pop()
        left, right = int(tree[k, 1]), int(tree[k, 2])
        if (left | right) == -1:
            seen[leaf[int(data[k, 6]):int(data[k, 7])]] = True
        else:
            stack += [left, right]
    return seen


def in_scene(b):
    """{3, 7} for the reference: the triangles no leaf names collapsed to a point (module text)"""
    def make():
        t = np.array(b[3], f32).reshape(-1, 40)
        out = ~referenced(b)
        t[out, 4:7] = t[out, 0:3]; t[out, 8:11] = t[out, 0:3]
        return b[3], {3: t.reshape(-1), 7: b[7]}
    return _once(("in_scene", _id(b[3]), _id(b[10])), make)[1]


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _regular(o, d):
    """float32 rays with finite, non-zero components (the irregular rays stay with the bit-parity tests)"""
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    d = np.where(d == 0, f32(1e-3), d)
    o = np.where(o == 0, f32(1e-3), o)
    assert np.isfinite(o).all() and np.isfinite(d).all() and (d != 0).all() and (o != 0).all()
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def rays(case, kind, n=N_RAYS, seed=3):
    """random: test_intersect_parity's cloud around the camera.  interior / edges / vertices: aimed at points of the scene's triangles — well
    inside one, on an edge, at a vertex —, half of them from the cloud around the camera and half from points about the scene's box.
    ellipsoids: random, a quarter starting in or near an ellipsoid, half of those aimed at one (test_gpu_parity's mixed rays, the regular part)."""
    def make():
        b = case.buffers
        rs = np.random.RandomState(seed + 17 * (SETS + ["ellipsoids"]).index(kind))
        cam = np.array(b[0], np.float64)
        o = cam + rs.normal(scale=0.3, size=(n, 3))
        d = _unit(rs.normal(size=(n, 3)))
        if kind == "ellipsoids":
            e = np.asarray(b[7]); ne = int(e[0])
            c = e[1:1 + 3 * ne].reshape(ne, 3); rad = e[1 + 9 * ne:1 + 10 * ne]
            k = np.arange(0, n, 4)
            which = rs.randint(0, ne, size=k.size)
            o[k] = c[which] + rs.normal(size=(k.size, 3)) * rad[which, None] * rs.choice([0.3, 1.0, 2.5], size=(k.size, 1))
            k2 = np.arange(1, n, 8)
            d[k2] = _unit(c[rs.randint(0, ne, size=k2.size)] + rs.normal(scale=0.05, size=(k2.size, 3)) - o[k2])
        elif kind != "random":
            v1, v2, v3 = R64.vertices(in_scene(b))
            area = np.linalg.norm(np.cross(v2 - v1, v3 - v1), axis=1)
            ids = np.nonzero(area > 0)[0]
            lo, hi = np.minimum.reduce([v1[ids], v2[ids], v3[ids]]).min(axis=0), np.maximum.reduce([v1[ids], v2[ids], v3[ids]]).max(axis=0)
            far = np.arange(n) % 2 == 1
            o[far] = (0.5 * (lo + hi) + rs.uniform(-0.75, 0.75, size=(n, 3)) * (hi - lo + 0.5))[far]
            k = ids[rs.randint(0, ids.size, size=n)]
            if kind == "interior":
                w = rs.dirichlet((1.0, 1.0, 1.0), size=n) * 0.7 + 0.1          # every weight in [0.1, 0.8]
            elif kind == "edges":
                s = rs.uniform(0.05, 0.95, size=n)
                w = np.zeros((n, 3)); w[:, 0] = s; w[:, 1] = 1.0 - s
                w = np.take_along_axis(w, (np.arange(3)[None, :] + rs.randint(0, 3, size=(n, 1))) % 3, axis=1)
            else:
                w = np.eye(3)[rs.randint(0, 3, size=n)]
            target = w[:, 0:1] * v1[k] + w[:, 1:2] * v2[k] + w[:, 2:3] * v3[k]
            d = _unit(target - o)
        return _regular(o, d)
    return _once(("rays", case.name, _id(case.buffers[3]), kind, n, seed), make)


def reference(case, kind, n=N_RAYS, seed=3):
    """(o, d, Hit) of a ray set in a scene, computed once"""
    def make():
        o, d = rays(case, kind, n, seed)
        return o, d, R64.closest_hit(in_scene(case.buffers), o, d)
    return _once(("ref", case.name, _id(case.buffers[3]), kind, n, seed), make)


def oracle_hits(oracle, case, o, d):
    """oracle.ray_hits in pt_debug_intersect's form: (tuv float32 (n, 3), prim int32) — prim -1 on a miss"""
    def make():
        tuv, code = oracle.ray_hits(oracle.Scene(case.buffers, case.tex[0], {k: v for k, v in case.tex.items() if k != 0}), o, d)
        typ, pid = code >> 24, code & 0xFFFFFF
        prim = np.where(code < 0, -1, np.where(typ == 1, pid, R64.PRIM_ELLIPSOID | pid)).astype(np.int32)
        return o, d, tuv, prim
    return _once(("oracle", case.name, _id(case.buffers[3]), _id(case.buffers[10]), _id(o), _id(d)), make)[2:]


def unit(ref, o):
    """the length the bound is a multiple of, per ray: 2^-24 (|o|_inf + |t| + extent) / |n . d|"""
    t = np.where(ref.hit(), np.abs(ref.t), 0.0)
    return 2.0 ** -24 * (np.abs(np.asarray(o, np.float64)).max(axis=1) + t + ref.extent) / ref.cos


def multiples(ref, o, tuv, prim):
    """per ray the largest of |t - t_ref|, |u - u_ref|, |v - v_ref| in units of unit() — t alone where an ellipsoid wins (the kernels keep other
    words in its u and v) —, 0 where nothing is hit; rays on which prim differs from the reference's are the caller's to exclude"""
    tuv = np.asarray(tuv, np.float64)
    un = unit(ref, o)
    m = np.abs(tuv[:, 0] - ref.t) / un
    tri = ref.hit() & ((ref.prim & R64.PRIM_ELLIPSOID) == 0)
    m = np.where(tri, np.maximum.reduce([m, np.abs(tuv[:, 1] - ref.u) / un, np.abs(tuv[:, 2] - ref.v) / un]), m)
    return np.where(ref.hit(), m, 0.0)


def missed(tuv, prim):
    """a hit record that says `no hit`, as test_intersect_parity reads it"""
    return (prim == -1) | ~(tuv[:, 0] < 1e25)


def same_prim(ref, tuv, prim):
    """bool per ray: the record names the reference's primitive (or both name none)"""
    none = missed(tuv, prim)
    return np.where(ref.hit(), ~none & (prim == ref.prim), none)
