"""CPU: the float64 brute-force closest hit of tests/_intersect_ref64.py against the reference of record, oracle.ray_scene's rayBVH (through
oracle.ray_hits, which also returns rayTri's u and v).  Here the reference's criteria are shown to hold for the oracle: on every robust ray the
two name the same primitive, with no exception, and t, u, v lie within the bound; the robust share of the random and the interior-aimed sets is
at least 95 %; and a tree damaged on purpose is noticed.

Measured here (4096 rays per set; scenes and sets of tests/_intersect_cases.py: C1, C1rot, C2, C3, C5 at subdiv 2, C6 with 24 and with 70 groups,
the eight moved scenes on refit trees, M1 at step 4, M5 at steps 3 and 7 — 77 sets, 315 392 rays):
  disagreements on robust rays     0
  robust share, random sets        97.8 % (C6 with 70 groups) to 100 %
  robust share, interior sets      96.2 % (soup1000) to 100 %
  robust share, edge / vertex sets 0 % (emptyleaf: every target is on the boundary of the one triangle) to 77 %; the oracle and the reference
                                   disagree on 239 to 1342 of 4096 such rays, all of them non-robust: float32 rayTri deciding the other way
                                   on a boundary
  K, the largest of |t - t_ref|, |u - u_ref|, |v - v_ref| over a robust ray's unit 2^-24 (|o|_inf + |t| + extent) / |n . d|
                                   203.6 (u of an interior-aimed ray of soup257; t alone: 44.3)
  the bound                        BOUND_K = 4 K = 814.4 units
With the edge margin at a flat 1e-4 (no term for float32's own rounding of u and v) 38 robust rays of the edge- and vertex-aimed sets of the
soups, objects70, leafroot, ladder60 and M5 disagreed, every one on a triangle the ray grazes (|det| below 0.5 % of |e1| |e2| |d|) with u, v or
u + v between 1.1e-4 and 8e-4 from a boundary: float32's u there is good to about 1e-3 only.  Hence the rounding term (_intersect_ref64's text)."""
import numpy as np
import pytest

import _intersect_cases as IC
import _intersect_ref64 as R64

f32 = np.float32
SHARE = 0.95
CASES = [("static", n) for n in ("C1", "C1rot", "C2", "C3", "C5", "C6", "C6g70")] + [("moved", n) for n in IC.MOVED] + [("M1", 4), ("M5", 3), ("M5", 7)]
_seen = {}


def case_of(pt, kind, arg):
    if kind == "static":
        return IC.static(pt, arg)
    return {"moved": IC.moved, "M1": IC.m1, "M5": IC.m5}[kind](pt, arg)[1]


def sets_of(case):
    return IC.SETS + (["ellipsoids"] if int(case.buffers[7][0]) else [])


def compare(oracle, case, kind):
    """-> (robust share, largest multiple of the unit on a robust ray); asserts the zero-exception criterion and the bound"""
    key = (case.name, kind)
    if key not in _seen:
        o, d, ref = IC.reference(case, kind)
        tuv, prim = IC.oracle_hits(oracle, case, o, d)
        assert ref.slivers == 0
        robust = ref.robust()
        same = IC.same_prim(ref, tuv, prim)
        bad = np.nonzero(robust & ~same)[0]
        assert bad.size == 0, (key, bad.size, [(int(i), int(ref.prim[i]), float(ref.t[i]), int(prim[i]), tuv[i].tolist()) for i in bad[:4]])
        m = IC.multiples(ref, o, tuv, prim)[robust]
        k = float(m.max()) if m.size else 0.0
        print(f"{case.name} {kind}: hits {ref.hit().mean():.3f}, robust {robust.mean():.4f}, differing non-robust rays {int((~same).sum())}, K {k:.2f}")
        assert k <= IC.BOUND_K, (key, k)
        _seen[key] = (float(robust.mean()), k)
    return _seen[key]


@pytest.mark.parametrize("kind,arg", CASES, ids=[f"{k}-{a}" for k, a in CASES])
def test_oracle_equals_the_reference_on_every_robust_ray(pt, oracle, kind, arg):
    case = case_of(pt, kind, arg)
    for rays in sets_of(case):
        share, _ = compare(oracle, case, rays)
        if rays in ("random", "interior"):
            assert share >= SHARE, (case.name, rays, share)       # a condition on the inputs: a scene that misses it needs other rays, not another threshold


def test_the_recorded_k_is_the_measured_one(pt, oracle):
    k = max(compare(oracle, case_of(pt, kind, arg), rays)[1] for kind, arg in CASES for rays in sets_of(case_of(pt, kind, arg)))
    assert 0.99 * IC.MEASURED_K <= k <= IC.MEASURED_K and IC.BOUND_K == 4.0 * IC.MEASURED_K, k


def test_matrix_form_equals_the_textbook_form(pt):
    """closest_hit's (rays, triangles) products against moller_trumbore() for the winner of each of 256 rays, and the rule applied one triangle at a time for 16 of them"""
    case = IC.static(pt, "C5")
    o, d, ref = IC.reference(case, "interior")
    v1, v2, v3 = R64.vertices(IC.in_scene(case.buffers))
    oo = o.astype(np.float64) + 1e-4 * d.astype(np.float64)
    for i in range(256):
        k = int(ref.prim[i])
        assert k >= 0
        det, u, v, t = R64.moller_trumbore(oo[i], d[i], v1[k], v2[k], v3[k])
        assert abs(u - ref.u[i]) < 1e-11 and abs(v - ref.v[i]) < 1e-11 and abs(t - ref.t[i]) < 1e-11 * max(1.0, t)
    for i in range(16):
        best, who = 1e30, -1
        for k in range(len(v1)):
            det, u, v, t = R64.moller_trumbore(oo[i], d[i], v1[k], v2[k], v3[k])
            if abs(det) >= 1e-10 and 0.0 <= u <= 1.0 and v >= 0.0 and u + v <= 1.0 and t > 1e-10 and t < best:
                best, who = t, k
        assert who == ref.prim[i] or not ref.robust()[i]


def test_ellipsoid_rule_inside_outside_and_rotated():
    """one sphere of radius 1 at the origin: from outside the near root, from inside the negative near root, beside it nothing; a
    stretched ellipsoid turned a quarter about z has its long axis where the rotation puts it"""
    none = np.zeros(0, f32)
    sphere = {3: none, 7: np.array([1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 1, 0], f32)}
    o = np.array([[0, 0, -3], [0, 0, 0.5], [0, 2, -3], [0, 0, 3]], f32)
    d = np.array([[0, 0, 1]] * 4, f32)
    h = R64.closest_hit(sphere, o, d)
    assert h.prim.tolist() == [R64.PRIM_ELLIPSOID, R64.PRIM_ELLIPSOID, -1, -1]
    assert abs(h.t[0] - (2.0 - 1e-4)) < 1e-12 and abs(h.t[1] - (-1.5 - 1e-4)) < 1e-12 and h.t[2] == 1e30
    # x^2 / 4 + y^2 + z^2 = 1 (f = 0.25) reaches x = 2 and y = 1; with rot.z = pi / 2 the frame sees p @ RZ = (-p.y, p.x, p.z): the long axis lies along y
    long_x = {3: none, 7: np.array([1, 0, 0, 0, 0.25, 1, 1, 0, 0, 0, 1, 0], f32)}
    turned = {3: none, 7: np.array([1, 0, 0, 0, 0.25, 1, 1, 0, 0, np.pi / 2, 1, 0], f32)}
    o = np.array([[1.5, 0, -3], [0, 1.5, -3]], f32); d = np.array([[0, 0, 1]] * 2, f32)
    assert R64.closest_hit(long_x, o, d).prim.tolist() == [R64.PRIM_ELLIPSOID, -1]
    assert R64.closest_hit(turned, o, d).prim.tolist() == [-1, R64.PRIM_ELLIPSOID]


# ------------------------------------------------------------------------------------------------ the check has teeth

def path_to(b, tri):
    """the node ids from a root of binding 13 down to the leaf whose range names triangle `tri`"""
    tree = np.asarray(b[11], np.int32).reshape(-1, 3)
    data = np.asarray(b[10], f32).reshape(-1, 8)
    leaf = np.asarray(b[12], np.int32)
    stack = [[int(r)] for r in np.asarray(b[13], np.int32)[1:1 + int(b[13][0])]]
    while stack:
        path = stack.pop()
        k = path[-1]
        left, right = int(tree[k, 1]), int(tree[k, 2])
        if (left | right) == -1:
            if tri in leaf[int(data[k, 6]):int(data[k, 7])]:
                return path
        else:
            stack += [path + [left], path + [right]]
    raise AssertionError("no leaf names the triangle")


@pytest.mark.parametrize("which", ["inner", "leaf"])
def test_a_box_too_small_is_noticed(pt, oracle, which):
    """C3's binding 10 with one node's max lowered below a triangle it covers — an inner node half way down the path, or the leaf itself: rays
    aimed at the triangle's interior that pass the shrunken box by no longer find it in the oracle, and the reference, which reads no box, says so.
    (Damaged trees run on the CPU oracle only.)"""
    case = IC.static(pt, "C3")
    b = case.buffers
    v1, v2, v3 = R64.vertices(b)
    _, _, seen = IC.reference(case, "interior")
    from_camera = seen.robust() & (np.arange(seen.prim.size) % 2 == 0)
    by_hits = np.argsort(-np.bincount(seen.prim[from_camera], minlength=len(v1)), kind="stable")
    tri, path = next((int(k), path_to(b, int(k))) for k in by_hits if len(path_to(b, int(k))) >= 6)      # the triangle the camera's rays find most often, among those deep in a tree
    assert seen.prim[from_camera].tolist().count(tri) > 0
    node = path[-1] if which == "leaf" else path[len(path) // 2]
    lowest = np.minimum.reduce([v1[tri], v2[tri], v3[tri]])
    data = np.array(b[10], f32).reshape(-1, 8)
    assert (data[node, 3:6] >= np.maximum.reduce([v1[tri], v2[tri], v3[tri]]).astype(f32)).all()      # it covers the triangle now
    data[node, 3:6] = np.minimum(data[node, 3:6], (lowest - 1e-3).astype(f32))
    damaged = dict(b); damaged[10] = data.reshape(-1)
    rs = np.random.RandomState(5)
    n = 1024
    w = rs.dirichlet((1.0, 1.0, 1.0), size=n) * 0.7 + 0.1
    target = w[:, 0:1] * v1[tri] + w[:, 1:2] * v2[tri] + w[:, 2:3] * v3[tri]
    o = np.array(b[0], np.float64) + rs.normal(scale=0.3, size=(n, 3))
    d = target - o
    o, d = IC._regular(o, d / np.linalg.norm(d, axis=1, keepdims=True))
    ref = R64.closest_hit(IC.in_scene(b), o, d)
    robust = ref.robust()
    aimed = robust & (ref.prim == tri)
    assert aimed.sum() > n // 4, int(aimed.sum())
    sound = IC.oracle_hits(oracle, case, o, d)
    assert IC.same_prim(ref, *sound)[robust].all()
    broken = IC.oracle_hits(oracle, IC.Case(f"C3 damaged {which}", damaged, case.tex, case.size), o, d)
    differ = robust & ~IC.same_prim(ref, *broken)
    assert (differ & aimed).sum() > aimed.sum() // 10, (int(differ.sum()), int(aimed.sum()))
