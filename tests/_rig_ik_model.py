"""include/pt_rig_ik.h's rule in numpy binary32, written from the header and not from the C++: every value is a float32 scalar or array and every
numpy operation rounds once, so a * b + c below is a rounded product and a rounded sum, in the order written.  One constraint at a time, as the
header states the rule.  The world matrices are tests/_rig_model.py's (include/pt_rig.h), imported and not copied.  Also the cases the tests of
the solve share, and the packers of constraints and goals."""
import numpy as np

import _rig_model as RM

f32 = np.float32
ZERO, ONE, TWO = f32(0), f32(1), f32(2)
TWO_BONE, AIM, POLE = 0, 1, 1
FLT_MAX = np.finfo(f32).max
CONSTRAINT = np.dtype([("kind", np.int32), ("joint", np.int32), ("flags", np.int32), ("pad", np.int32), ("axis", f32, 3), ("padf", f32)])
GOAL = np.dtype([("target", f32, 3), ("weight", f32), ("pole", f32, 3), ("padf", f32)])


def two_bone(tip, pole=False):
    return dict(kind=TWO_BONE, joint=int(tip), flags=POLE if pole else 0, axis=(0.0, 0.0, 0.0))


def aim(joint, axis):
    return dict(kind=AIM, joint=int(joint), flags=0, axis=tuple(float(x) for x in axis))


def goal(target, weight=1.0, pole=(0.0, 0.0, 0.0)):
    return dict(target=np.asarray(target, f32), weight=f32(weight), pole=np.asarray(pole, f32))


def pack_constraints(cons):
    out = np.zeros(len(cons), CONSTRAINT)
    for i, c in enumerate(cons):
        out[i] = (c["kind"], c["joint"], c["flags"], 0, np.asarray(c["axis"], f32), 0.0)
    return out


def pack_goals(goals):
    out = np.zeros(len(goals), GOAL)
    for i, g in enumerate(goals):
        out[i] = (g["target"], g["weight"], g["pole"], 0.0)
    return out


def ok(x):
    return bool(x != 0 and abs(x) <= FLT_MAX)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def length(a):
    return np.sqrt(dot(a, a))


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], f32)


def unit(q):
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return (q / n).astype(f32)


def rot(q):
    x, y, z, w = q
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return np.array([[ONE - TWO * (yy + zz), TWO * (xy - wz), TWO * (xz + wy)],
                     [TWO * (xy + wz), ONE - TWO * (xx + zz), TWO * (yz - wx)],
                     [TWO * (xz - wy), TWO * (yz + wx), ONE - TWO * (xx + yy)]], f32)


def apply(M, v):
    return ((M[:, 0] * v[0] + M[:, 1] * v[1]) + M[:, 2] * v[2]).astype(f32)


def qmul(p, q):
    return np.array([((p[3] * q[0] + p[0] * q[3]) + p[1] * q[2]) - p[2] * q[1],
                     ((p[3] * q[1] - p[0] * q[2]) + p[1] * q[3]) + p[2] * q[0],
                     ((p[3] * q[2] + p[0] * q[1]) - p[1] * q[0]) + p[2] * q[3],
                     ((p[3] * q[3] - p[0] * q[0]) - p[1] * q[1]) - p[2] * q[2]], f32)


def from_to(u, v):
    """step 4, the fallback axis included"""
    m = u + v
    ml = length(m)
    if ml == 0:
        k = np.array([ZERO, u[2], -u[1]], f32)
        kl = length(k)
        if kl == 0:
            return np.array([0, 0, 1, 0], f32)
        return np.array([k[0] / kl, k[1] / kl, k[2] / kl, ZERO], f32)
    mh = m / ml
    c = cross(u, mh)
    return np.array([c[0], c[1], c[2], dot(u, mh)], f32)


def frame(P):
    """step 1: (cofactors, det, translation) of the 3 x 4 P, or None for a first joint that is a root"""
    if P is None:
        return None
    c = np.zeros((3, 3), f32)
    for i in range(3):
        for k in range(3):
            i1, i2, k1, k2 = (i + 1) % 3, (i + 2) % 3, (k + 1) % 3, (k + 2) % 3
            c[i, k] = P[i1, k1] * P[i2, k2] - P[i1, k2] * P[i2, k1]
    det = (P[0, 0] * c[0, 0] + P[0, 1] * c[0, 1]) + P[0, 2] * c[0, 2]
    return c, det, P[:, 3].copy()


def into_frame(F, x):
    if F is None:
        return x.copy()
    c, det, p3 = F
    d = x - p3
    return np.array([((c[0, k] * d[0] + c[1, k] * d[1]) + c[2, k] * d[2]) / det for k in range(3)], f32)


def weighted(n, qs, e):
    if e == 1:
        return qs.copy()
    v = ONE - e
    d = ((n[0] * qs[0] + n[1] * qs[1]) + n[2] * qs[2]) + n[3] * qs[3]
    eq = -e if d < 0 else e
    return (v * n + eq * qs).astype(f32)


def solve_two_bone(P, root, mid, tip_t, g, use_pole, trace=None, mutate=None):
    """steps 0-4, 6, 7: (q_root, q_mid) or None when the joints stay.  mutate: "sin" negates sinA, "swap" swaps l1 and l2 in the cosine rule"""
    target, e = g["target"], f32(g["weight"])
    if e == 0 or np.isnan(target).any():
        return None
    F = frame(P)
    gF = into_frame(F, target)
    n0, n1 = unit(root[4:8]), unit(mid[4:8])
    L0, L1 = rot(n0) * root[None, 8:11], rot(n1) * mid[None, 8:11]
    a = root[0:3]
    b = apply(L0, mid[0:3]) + a
    c = apply(L0, apply(L1, tip_t) + mid[0:3]) + a
    e1, e2, v = b - a, c - b, gF - a
    l1, l2, dist = length(e1), length(e2), length(v)
    eh = v / dist
    lo, hi = abs(l1 - l2), l1 + l2
    d = lo if dist < lo else dist
    d = hi if d > hi else d
    ca, cb = (l2, l1) if mutate == "swap" else (l1, l2)
    cosA = ((ca * ca + d * d) - cb * cb) / ((TWO * ca) * d)
    cosA = -ONE if cosA < -1 else cosA
    cosA = ONE if cosA > 1 else cosA
    sinA = np.sqrt(ONE - cosA * cosA)
    if mutate == "sin":
        sinA = -sinA
    h0 = into_frame(F, g["pole"]) - a if use_pole else e1
    h = h0 - eh * dot(h0, eh)
    hl = length(h)
    hh = h / hl
    u1 = cosA * eh + sinA * hh
    bp, cp = a + l1 * u1, a + d * eh
    r1 = from_to(e1 / l1, u1)
    e2p = apply(rot(r1), e2)
    l2p = length(e2p)
    w = cp - bp
    wl = length(w)
    r2 = from_to(e2p / l2p, w / wl)
    q0 = qmul(r1, n0)
    conj = np.array([-q0[0], -q0[1], -q0[2], q0[3]], f32)
    q1 = qmul(qmul(qmul(conj, r2), q0), n1)
    if trace is not None:
        trace.update(l1=l1, l2=l2, dist=dist, d=d, hl=hl, l2p=l2p, wl=wl, det=ONE if F is None else F[1], cosA=cosA, m1=length(e1 / l1 + u1), m2=length(e2p / l2p + w / wl))
    if not all(ok(x) for x in (ONE if F is None else F[1], l1, l2, dist, hl, l2p, wl)):
        return None
    return weighted(n0, q0, e), weighted(n1, q1, e)


def solve_aim(P, j, axis, g, trace=None):
    target, e = g["target"], f32(g["weight"])
    if e == 0 or np.isnan(target).any():
        return None
    F = frame(P)
    gF = into_frame(F, target)
    n = unit(j[4:8])
    u = apply(rot(n), np.asarray(axis, f32))
    w = gF - j[0:3]
    wl = length(w)
    q = qmul(from_to(u, w / wl), n)
    if trace is not None:
        trace.update(wl=wl, det=ONE if F is None else F[1], m=length(u + w / wl))
    if not (ok(ONE if F is None else F[1]) and ok(wl)):
        return None
    return weighted(n, q, e)


def ik_locals(parent, cons, goals, locals_, traces=None, mutate=None):
    """the rule over a table: (n, 12) float32.  goals None: off"""
    parent = np.asarray(parent, np.int64)
    l = np.ascontiguousarray(locals_, f32).reshape(-1, 12)
    out = l.copy()
    if goals is None or not len(cons):
        return out
    with np.errstate(all="ignore"):
        W = RM.world(parent, l)
        for k, (c, g) in enumerate(zip(cons, goals)):
            trace = {} if traces is not None else None
            j = c["joint"]
            if c["kind"] == AIM:
                first = j
                P = W[parent[first]] if parent[first] >= 0 else None
                q = solve_aim(P, l[j], c["axis"], g, trace)
                if q is not None:
                    out[j, 4:8] = q
            else:
                mid = parent[j]
                first = parent[mid]
                P = W[parent[first]] if parent[first] >= 0 else None
                q = solve_two_bone(P, l[first], l[mid], l[j, 0:3], g, bool(c["flags"] & POLE), trace, mutate)
                if q is not None:
                    out[first, 4:8], out[mid, 4:8] = q
            if traces is not None:
                trace["written"] = q is not None
                traces.append(trace)
    return out


def ik_records(parent, cons, goals, locals_, inv_bind=None):
    return RM.records(parent, ik_locals(parent, cons, goals, locals_), inv_bind)


def window(parent, cons):
    """(before, from): the levels [0, before) run ahead of the solve and [from, levels) after it"""
    if not len(cons):
        return 0, 0
    parent = np.asarray(parent, np.int64)
    d = RM.depths(parent)
    firsts = [c["joint"] if c["kind"] == AIM else parent[parent[c["joint"]]] for c in cons]
    levels = [int(d[j]) - 1 for j in firsts]
    return max(levels), min(levels)


def independent(parent, cons):
    """the header's condition, literally: for A != B, W(A) and R(B) do not meet"""
    parent = np.asarray(parent, np.int64)
    Ws, Rs = [], []
    for c in cons:
        j = c["joint"]
        own = [j] if c["kind"] == AIM else [parent[parent[j]], parent[j], j]
        Ws.append(set(own[:1] if c["kind"] == AIM else own[:2]))
        r, a = set(own), parent[own[0]]
        while a >= 0:
            r.add(a)
            a = parent[a]
        Rs.append(r)
    return all(not (Ws[a] & Rs[b]) for a in range(len(cons)) for b in range(len(cons)) if a != b)


# ------------------------------------------------------------------------------------------------ the cases

def rigid_locals(n, seed, shift=1.0, unnormalised=True):
    """locals with a uniform scale per joint (a rigid chain under a similarity), NaN in the paddings"""
    l = RM.random_locals(n, seed, scale=(0.7, 1.4), shift=shift, unnormalised=unnormalised)
    l[:, 9] = l[:, 8]
    l[:, 10] = l[:, 8]
    return l


def chain_geometry(parent, locals_, tip):
    """binary64: (a, l1, l2, A, p) of the chain ending in tip: the chain root's world position, the bone lengths in world space, and the linear part
    and translation of the world matrix of the root's parent (identity and 0 for a rig's root)"""
    parent = np.asarray(parent, np.int64)
    W = world64(parent, locals_)
    mid = parent[tip]
    root = parent[mid]
    pos = lambda j: W[j][:, 3]
    P = W[parent[root]] if parent[root] >= 0 else np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    return pos(root), np.linalg.norm(pos(mid) - pos(root)), np.linalg.norm(pos(tip) - pos(mid)), P[:, :3], P[:, 3]


def world64(parent, locals_):
    """include/pt_rig.h steps 1 and 2 in binary64 from the binary32 locals: (n, 3, 4)"""
    parent = np.asarray(parent, np.int64)
    l = np.asarray(locals_, np.float64).reshape(-1, 12)
    W = np.zeros((l.shape[0], 3, 4))
    for j in range(l.shape[0]):
        x, y, z, w = l[j, 4:8] / np.linalg.norm(l[j, 4:8])
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        L = np.concatenate([R * l[j, None, 8:11], l[j, 0:3, None]], axis=1)
        if parent[j] < 0:
            W[j] = L
        else:
            A = W[parent[j]]
            W[j, :, :3] = A[:, :3] @ L[:, :3]
            W[j, :, 3] = A[:, :3] @ L[:, 3] + A[:, 3]
    return W


def reach_target(parent, locals_, tip, rng, frac=None, direction=None):
    """a world-space target for the chain ending in tip at a reach drawn from [1.05 |l1 - l2|, 0.95 (l1 + l2)] (or at frac of that span), float32"""
    a, l1, l2, _, _ = chain_geometry(parent, locals_, tip)
    lo, hi = 1.05 * abs(l1 - l2), 0.95 * (l1 + l2)
    reach = rng.uniform(lo, hi) if frac is None else lo + frac * (hi - lo)
    d = rng.normal(size=3) if direction is None else np.asarray(direction, np.float64)
    return (a + d / np.linalg.norm(d) * reach).astype(f32)


HUMANOID = np.array([-1, 0, 1, 2, 3, 2, 5, 6, 2, 8, 9, 0, 11, 12, 0, 14, 15], np.int32)      # spine 0-1-2, head 3-4, arms 5-6-7 and 8-9-10, legs 11-12-13 and 14-15-16


def _case(tag, parent, locals_, cons, goals, bind_seed=None):
    parent = np.asarray(parent, np.int32)
    return dict(tag=tag, parent=parent, locals=np.ascontiguousarray(locals_, f32), cons=cons, goals=goals,
                bind=None if bind_seed is None else RM.random_binds(parent.size, bind_seed))


def ik_cases():
    """the cases the GPU test and the C++ check share, each dict(tag, parent, locals, cons, goals, bind)"""
    out = []
    rng = np.random.RandomState(11)
    # a 3-joint rig whose chain root is the rig's root (no P); weights 0, 1 and 0.37; with and without a pole
    p3 = RM.chain(3)
    l3 = rigid_locals(3, 1)
    t3 = reach_target(p3, l3, 2, rng)
    for w in (1.0, 0.37, 0.0):
        for pole in (False, True):
            out.append(_case(f"root chain w{w} pole{int(pole)}", p3, l3, [two_bone(2, pole)], [goal(t3, w, (0.3, 2.0, -1.0))]))
    # 4 joints: a parent with scale and rotation
    p4 = RM.chain(4)
    l4 = rigid_locals(4, 2)
    l4[0, 8:11] = (1.7, 1.7, 1.7)
    for pole in (False, True):
        out.append(_case(f"under a parent pole{int(pole)}", p4, l4, [two_bone(3, pole)], [goal(reach_target(p4, l4, 3, rng), 1.0, (1.0, -2.0, 0.5))], bind_seed=5))
    out.append(_case("under a non-uniform parent", p4, RM.random_locals(4, 3), [two_bone(3, True)], [goal(reach_target(p4, RM.random_locals(4, 3), 3, rng), 0.37, (1.0, -2.0, 0.5))]))
    # the reach: beyond, inside |l1 - l2|, at full extension (a target along the chain's own extended line is left alone without a pole: with one)
    a, l1, l2, A, p = chain_geometry(p4, l4, 3)
    way = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    for name, r in (("beyond", 3.0 * (l1 + l2)), ("inside", 0.3 * abs(l1 - l2)), ("full", l1 + l2)):
        for pole in (False, True):
            out.append(_case(f"reach {name} pole{int(pole)}", p4, l4, [two_bone(3, pole)], [goal((a + way * r).astype(f32), 1.0, (1.0, -2.0, 0.5))]))
    # two chains whose roots lie at depths 1 and 3 (levels 0 and 2): the window overlaps
    # (the shallow chain hangs under a parent, so that the second pass starts below level 0 too: levels [0, 3), the solve, levels [1, end); the
    # deeper chain hangs under a second root, so that neither reads what the other writes)
    p10 = np.array([-1, 0, 1, 2, -1, 4, 5, 6, 7, 8], np.int32)
    l10 = rigid_locals(10, 4)
    c10 = [two_bone(3), two_bone(9, True)]
    assert window(p10, c10) == (3, 1)
    out.append(_case("two depths", p10, l10, c10, [goal(reach_target(p10, l10, 3, rng), 1.0), goal(reach_target(p10, l10, 9, rng), 0.37, (0.0, 3.0, 0.0))], bind_seed=6))
    # mixed kinds on a humanoid: two arms, two legs... and a head on one spine; unnormalised quaternions
    lh = rigid_locals(17, 5)
    ch = [two_bone(7, True), aim(3, (0.0, 0.0, 1.0)), two_bone(10), two_bone(13, True), aim(15, (0.6, 0.0, 0.8))]
    gh = [goal(reach_target(HUMANOID, lh, 7, rng), 1.0, (0.0, 5.0, 0.0)), goal((2.0, 1.0, -3.0), 0.37), goal(reach_target(HUMANOID, lh, 10, rng), 0.37),
          goal(reach_target(HUMANOID, lh, 13, rng), 1.0, (1.0, 0.0, 4.0)), goal((-1.0, 0.5, 0.25), 1.0)]
    out.append(_case("mixed kinds", HUMANOID, lh, ch, gh, bind_seed=7))
    out.append(_case("mixed kinds, weights 0", HUMANOID, lh, ch, [goal(g["target"], 0.0, g["pole"]) for g in gh]))
    # 65 constraints: a wave boundary is crossed.  65 three-joint chains under one root, every third an aim on the chain's first joint instead
    n = 1 + 65 * 3
    p65 = np.zeros(n, np.int32)
    p65[0] = -1
    for k in range(65):
        p65[1 + 3 * k: 4 + 3 * k] = (0, 1 + 3 * k, 2 + 3 * k)
    l65 = rigid_locals(n, 8)
    c65, g65 = [], []
    for k in range(65):
        tip = 3 + 3 * k
        if k % 3 == 2:
            c65.append(aim(tip - 2, (0.0, 1.0, 0.0))); g65.append(goal(rng.uniform(-3, 3, 3), (1.0, 0.37, 0.0)[k % 5 % 3]))
        else:
            c65.append(two_bone(tip, k % 2 == 1)); g65.append(goal(reach_target(p65, l65, tip, rng), (1.0, 0.37)[k % 4 == 0], rng.uniform(-3, 3, 3)))
    out.append(_case("65 constraints", p65, l65, c65, g65, bind_seed=9))
    # 0 constraints, goals set (an empty array) and goals off
    out.append(_case("0 constraints", p4, l4, [], []))
    out.append(_case("goals off", p4, l4, [two_bone(3)], None))
    out += left_cases()
    return out


def left_cases():
    """step 7, every reason to leave a constraint as it is, one at a time, the exact antiparallel cases of fromTo, and a NaN target.  The joints are
    axis-aligned so that the zeros and the antiparallel sums are exact in binary32"""
    out = []
    ident = np.zeros(12, f32); ident[7] = 1; ident[8:11] = 1; ident[3] = ident[11] = np.nan

    def straight(n, step=(0.0, 1.0, 0.0)):
        l = np.tile(ident, (n, 1))
        l[1:, 0:3] = step
        return l
    p3, p4 = RM.chain(3), RM.chain(4)
    bent = straight(3)
    bent[2, 0:3] = (1.0, 0.0, 0.0)                                       # root at 0, mid at (0, 1, 0), tip at (1, 1, 0)
    up = (0.0, 0.0, 5.0)

    def tb(tag, parent, l, target, pole=None, tip=None):
        tip = len(parent) - 1 if tip is None else tip
        out.append(_case("left: " + tag, parent, l, [two_bone(tip, pole is not None)], [goal(target, 1.0, pole if pole is not None else (0, 0, 0))]))
    z = bent.copy(); z[1, 0:3] = 0
    tb("l1 is 0", p3, z, (1.0, 1.0, 0.0), up)
    z = bent.copy(); z[2, 0:3] = 0
    tb("l2 is 0", p3, z, (1.0, 1.0, 0.0), up)
    z = bent.copy(); z[1, 1] = np.inf
    tb("l1 is not finite", p3, z, (1.0, 1.0, 0.0), up)
    z = bent.copy(); z[2, 0] = np.nan
    tb("l2 is not finite", p3, z, (1.0, 1.0, 0.0), up)
    tb("dist is 0", p3, bent, (0.0, 0.0, 0.0), up)
    tb("dist is not finite", p3, bent, (np.inf, 0.0, 0.0), up)
    tb("the target is NaN", p3, bent, (0.5, np.nan, 0.0), up)
    tb("h is 0: the pole on the line to the target", p3, bent, (0.0, 1.5, 0.0), (0.0, 3.0, 0.0))
    tb("h is 0: no pole and the first bone on the line to the target", p3, bent, (0.0, 1.5, 0.0))
    tb("h is not finite: a NaN pole", p3, bent, (1.0, 0.5, 0.0), (np.nan, 0.0, 0.0))
    z = straight(4); z[3, 0:3] = (1.0, 0.0, 0.0); z[0, 8] = 0.0           # the parent's s.x is 0: det is 0
    tb("det is 0", p4, z, (1.0, 2.0, 0.0), up)
    z = straight(4); z[3, 0:3] = (1.0, 0.0, 0.0); z[0, 0] = np.inf        # the parent's translation: det is fine, g_F is not
    tb("g_F is not finite", p4, z, (1.0, 2.0, 0.0), up)
    z = straight(4); z[3, 0:3] = (1.0, 0.0, 0.0); z[0, 9] = np.inf
    tb("det is not finite", p4, z, (1.0, 2.0, 0.0), up)
    # |c' - b'| is 0 alone: a second bone below half an ulp of the first.  d clamps to l1, cosA is 1 and sinA 0, so b' == c' exactly, while
    # l2 and |e2'| are 1e-9 and every other length is ordinary
    z = bent.copy(); z[2, 0:3] = (1e-9, 0.0, 0.0)
    tb("wl is 0", p3, z, (1.0, 0.5, 0.0), up)
    # |e2'| is 0 alone, at the denormal boundary of dot(): e2 = (x, 0, 0) with x * x = 0.7 * 2^-149, which rounds up to the smallest denormal, so
    # l2 is not 0; r1 turns e2 across two axes, each square is below half that denormal and rounds to 0.  c' - b' comes out along one axis again
    # and keeps its length.  (The first bone is 2^-70, so that l2 is no small fraction of it and |c' - b'| is l2 to rounding.)
    L, x = f32(2.0 ** -70), f32(np.sqrt(0.7) * 2.0 ** -74.5)
    z = bent.copy(); z[1, 0:3] = (0.0, L, 0.0); z[2, 0:3] = (x, 0.0, 0.0)
    tb("l2p is 0", p3, z, (f32(0.9375) * L, f32(1.125) * L, 0.0), (-f32(2.0 ** -60), 0.0, 0.0))
    # a not finite one of either is always masked by an earlier check: a finite l2 means |e2| <= sqrt(FLT_MAX), which R(r1), of entries no
    # larger than about 3, cannot carry to infinity, and |c' - b'| is at most l1 + d <= 2 l1 + l2.  So they are reached through l2 here
    z = bent.copy(); z[1, 8:11] = 3e38; z[1, 4:8] = (0, 0, 0, 1)           # the mid's scale: e2 overflows in the product, l2 is infinite
    tb("l2 overflows", p3, z, (1.0, 1.0, 0.0), up)
    # the aim's two
    out.append(_case("left: aim at the joint itself", p3, bent, [aim(1, (0.0, 1.0, 0.0))], [goal((0.0, 1.0, 0.0))]))
    out.append(_case("left: aim at a NaN", p3, bent, [aim(1, (0.0, 1.0, 0.0))], [goal((0.0, np.nan, 0.0))]))
    z = straight(3); z[0, 10] = 0.0
    out.append(_case("left: aim under a det of 0", p3, z, [aim(1, (0.0, 1.0, 0.0))], [goal((3.0, 1.0, 0.0))]))
    # antiparallel, exactly: the aim's axis points away from the target; along X the second fallback
    out.append(_case("antiparallel: aim along -y", p3, bent, [aim(1, (0.0, 1.0, 0.0))], [goal((0.0, -4.0, 0.0))]))
    out.append(_case("antiparallel: aim along -x", p3, bent, [aim(2, (1.0, 0.0, 0.0))], [goal((-7.0, 1.0, 0.0), 0.37)]))
    # and in the chain: the first bone points along +y and must turn to -y exactly (target below the root, pole along x, l1 == l2 == d / 2 ... cosA = 1)
    z = straight(3)
    out.append(_case("antiparallel: the first bone turns over", p3, z, [two_bone(2, True)], [goal((0.0, -2.0, 0.0), 1.0, (3.0, 0.0, 0.0))]))
    return out
