"""include/pt_rig_ik.h's rule in float64 with a bound on |binary32 result - this| that is derived, not fitted.  It is NOT a second reading of
the header: its scalar dot, cross, apply and length on (value, bound) pairs have the same structure and association as tests/_rig_ik_model.py,
because the bound is carried operation by operation and must follow the operations the binary32 statement performs.  What it holds is the
arithmetic: that the binary32 model computes what these expressions mean, to rounding.  A misreading of the header shared by model and
reference would pass here; what guards against that is the property test (the tip reaches the target, the mid lies on the pole's side), which
knows nothing of the expressions.

The inputs are the binary32 locals, goals and axes.  P, the world matrix of the first joint's parent, is the binary32 model's (tests/_rig_model.py:
what the levels ahead of the solve leave on the device), taken as an exact input: the solve is a function of it.  The decisions (the clamps of the
triangle, the shorter arc of the weight's lerp) are taken on the float64 values; the cases keep away from their ties.

THE BOUND.  u = 2^-24.  Every quantity of the rule is carried as a pair (x, E_x) with |binary32 x - float64 x| <= E_x, by the forward analysis
of each operation the header writes, in the header's order and association.  With r the float64 result and D the bound of the exact operation
on perturbed operands, the rounding adds u (|r| + D):
    a + b:    D = E_a + E_b                                   a * b:   D = |a| E_b + |b| E_a + E_a E_b
    a / b:    D = (E_a + |r| E_b) / (|b| - E_b)                sqrt a:  D = E_a / (sqrt a + sqrt(a - E_a))
    a select takes the chosen operand's E; a negation and |.| keep E; an input has E = 0.
None of these is a first-order statement: the second-order terms are in them.  A quotient whose divisor may be 0 (|b| <= E_b) and a root whose
operand may be negative (a <= E_a) are not bounded (E = inf); the tests require that not to happen on their cases.  A factor 1.01 at the end
covers the difference between float64 and exact arithmetic in the reference itself.
The analysis is entrywise and takes every rounding as adversarial, through some fifty roots and quotients: the bound comes out some forty times
the largest error seen, which is what such an analysis costs and still decades below what a wrong formula moves.
The properties' tolerance follows from the bound: a rotation matrix is quadratic in its quaternion, so a quaternion of norm about 1 that is off
by dq (2-norm) turns a vector x into one off by at most 4 |dq| |x| after the normalisation; a chain's tip then misses by at most
    |A|_2 * (4 |E_root| (l1 + l2) + 4 |E_mid| l2)
in world space, A the linear part of P.  The solve works in the frame of the binary32 P, the float64 forward kinematics of the properties in that
of the float64 P: a tip at c_F in F lands |A64 - A32|_2 |c_F| + |p64 - p32| apart in the two, and the tolerance adds exactly that.  The float64
solve itself, carried forward under the binary32 P, is held to 1e-9."""
import numpy as np

import _rig_ik_model as IM
import _rig_mix_ref64 as X64
import _rig_model as RM

U = 2.0 ** -24


class B:
    """a float64 value with its bound against the binary32 evaluation"""
    __slots__ = ("x", "e")

    def __init__(self, x, e=0.0):
        self.x, self.e = float(x), float(e)

    @staticmethod
    def of(v):
        return v if isinstance(v, B) else B(v)

    @staticmethod
    def rounded(r, d):
        return B(r, d + U * (abs(r) + d))

    def __add__(self, o):
        o = B.of(o)
        return B.rounded(self.x + o.x, self.e + o.e)

    __radd__ = __add__

    def __neg__(self):
        return B(-self.x, self.e)

    def __sub__(self, o):
        return self + (-B.of(o))

    def __rsub__(self, o):
        return B.of(o) + (-self)

    def __mul__(self, o):
        o = B.of(o)
        return B.rounded(self.x * o.x, abs(self.x) * o.e + abs(o.x) * self.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = B.of(o)
        r = self.x / o.x
        if not abs(o.x) > o.e:
            return B(r, np.inf)
        return B.rounded(r, (self.e + abs(r) * o.e) / (abs(o.x) - o.e))

    def sqrt(self):
        r = np.sqrt(self.x)
        if not self.x > self.e:
            return B(r, np.inf)
        return B.rounded(r, self.e / (r + np.sqrt(self.x - self.e)))

    def __abs__(self):
        return B(abs(self.x), self.e)


def vec(a):
    return [B.of(x) for x in a]


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def length(a):
    return dot(a, a).sqrt()


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def unit(q):
    n = (((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]).sqrt()
    return [c / n for c in q]


def rot(q):
    x, y, z, w = q
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)], [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
            [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]


def apply(M, v):
    return [(M[i][0] * v[0] + M[i][1] * v[1]) + M[i][2] * v[2] for i in range(3)]


def qmul(p, q):
    """the header's four products and three sums per component, through _rig_mix_ref64's signed tensor"""
    out = []
    for c in range(4):
        terms = [(a, b, X64.QT[c, a, b]) for a in (3, 0, 1, 2) for b in range(4) if X64.QT[c, a, b]]      # in the header's order: w first
        acc = None
        for a, b, sign in terms:
            t = p[a] * q[b]
            acc = (t if sign > 0 else -t) if acc is None else (acc + t if sign > 0 else acc - t)
        out.append(acc)
    return out


def from_to(u, v):
    m = [u[i] + v[i] for i in range(3)]
    ml = length(m)
    assert ml.x > 1e-6, "the cases of the reference keep away from the antiparallel fallback"
    mh = [c / ml for c in m]
    c = cross(u, mh)
    return [c[0], c[1], c[2], dot(u, mh)]


def frame(P):
    if P is None:
        return None
    P = [[B(x) for x in row] for row in np.asarray(P, np.float64)]
    c = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for k in range(3):
            i1, i2, k1, k2 = (i + 1) % 3, (i + 2) % 3, (k + 1) % 3, (k + 2) % 3
            c[i][k] = P[i1][k1] * P[i2][k2] - P[i1][k2] * P[i2][k1]
    det = (P[0][0] * c[0][0] + P[0][1] * c[0][1]) + P[0][2] * c[0][2]
    return c, det, [P[i][3] for i in range(3)]


def into_frame(F, x):
    x = vec(np.asarray(x, np.float64))
    if F is None:
        return x
    c, det, p3 = F
    d = [x[i] - p3[i] for i in range(3)]
    return [((c[0][k] * d[0] + c[1][k] * d[1]) + c[2][k] * d[2]) / det for k in range(3)]


def weighted(n, qs, e):
    if e == 1:
        return qs
    v = 1.0 - B(e)
    d = sum(a.x * b.x for a, b in zip(n, qs))
    eq = B(-e if d < 0 else e)
    return [v * n[f] + eq * qs[f] for f in range(4)]


def two_bone(P, root, mid, tip_t, goal, use_pole, mutate=None):
    """(q_root (4,), q_mid (4,), E_root (4,), E_mid (4,), geometry) in float64 with the derived entrywise bounds.  mutate as the model's"""
    root, mid = np.asarray(root, np.float64), np.asarray(mid, np.float64)
    F = frame(P)
    g = into_frame(F, goal["target"])
    n0, n1 = unit(vec(root[4:8])), unit(vec(mid[4:8]))
    scale = lambda R, s: [[R[i][c] * B(s[c]) for c in range(3)] for i in range(3)]
    L0, L1 = scale(rot(n0), root[8:11]), scale(rot(n1), mid[8:11])
    a, tm, tt = vec(root[0:3]), vec(mid[0:3]), vec(np.asarray(tip_t, np.float64))
    add = lambda p, q: [p[i] + q[i] for i in range(3)]
    sub = lambda p, q: [p[i] - q[i] for i in range(3)]
    b = add(apply(L0, tm), a)
    c = add(apply(L0, add(apply(L1, tt), tm)), a)
    e1, e2, v = sub(b, a), sub(c, b), sub(g, a)
    l1, l2, dist = length(e1), length(e2), length(v)
    eh = [x / dist for x in v]
    lo, hi = abs(l1 - l2), l1 + l2
    d = lo if dist.x < lo.x else dist
    d = hi if d.x > hi.x else d
    ca, cb = (l2, l1) if mutate == "swap" else (l1, l2)
    cosA = ((ca * ca + d * d) - cb * cb) / ((2.0 * ca) * d)
    cosA = B(-1.0) if cosA.x < -1 else cosA
    cosA = B(1.0) if cosA.x > 1 else cosA
    sinA = (1.0 - cosA * cosA).sqrt()
    if mutate == "sin":
        sinA = -sinA
    h0 = sub(into_frame(F, goal["pole"]), a) if use_pole else e1
    along = dot(h0, eh)
    h = [h0[i] - eh[i] * along for i in range(3)]
    hl = length(h)
    hh = [x / hl for x in h]
    u1 = [cosA * eh[i] + sinA * hh[i] for i in range(3)]
    bp = [a[i] + l1 * u1[i] for i in range(3)]
    cp = [a[i] + d * eh[i] for i in range(3)]
    r1 = from_to([x / l1 for x in e1], u1)
    e2p = apply(rot(r1), e2)
    l2p = length(e2p)
    w = sub(cp, bp)
    wl = length(w)
    r2 = from_to([x / l2p for x in e2p], [x / wl for x in w])
    q0 = qmul(r1, n0)
    conj = [-q0[0], -q0[1], -q0[2], q0[3]]
    q1 = qmul(qmul(qmul(conj, r2), q0), n1)
    e = float(goal["weight"])
    q0, q1 = weighted(n0, q0, e), weighted(n1, q1, e)
    val = lambda q: np.array([c.x for c in q])
    err = lambda q: 1.01 * np.array([c.e for c in q])
    geo = dict(l1=l1.x, l2=l2.x, dist=dist.x, d=d.x, a=val(a), g=val(g), eh=val(eh), h0=val(h0))
    return val(q0), val(q1), err(q0), err(q1), geo


def solve(case, k=0, mutate=None):
    """the chain of constraint k of a case of _rig_ik_model: (q_root, q_mid, E_root, E_mid, geometry, (root, mid, tip))"""
    parent, l = np.asarray(case["parent"], np.int64), case["locals"]
    c, g = case["cons"][k], case["goals"][k]
    tip = c["joint"]
    mid = parent[tip]
    root = parent[mid]
    W = RM.world(parent, l)
    P = W[parent[root]] if parent[root] >= 0 else None
    return two_bone(P, l[root], l[mid], l[tip, 0:3], g, bool(c["flags"] & IM.POLE), mutate) + ((root, mid, tip),)


# ------------------------------------------------------------------------------------------------ the cases of the reference and the properties

def random_cases(count, seed=1):
    """rigid chains (a uniform scale per joint, unnormalised quaternions) of four joints under a scaled, rotated parent, every other one with a pole;
    the reach drawn from [1.05 |l1 - l2|, 0.95 (l1 + l2)], a pole at least 0.2 rad off the line to the target.  No case is left out: a pole that
    falls nearer is drawn again, before anything is solved"""
    rng = np.random.RandomState(seed)
    parent = RM.chain(4)
    out = []
    for it in range(count):
        l = IM.rigid_locals(4, 1000 + seed * 100000 + it)
        l[:, 0:3] *= np.float32(rng.uniform(0.3, 1.5))
        target = IM.reach_target(parent, l, 3, rng)
        use_pole = it % 2 == 1
        a = IM.chain_geometry(parent, l, 3)[0]
        pole = np.zeros(3, np.float32)
        while use_pole:
            pole = (a + rng.normal(size=3) * 2.0).astype(np.float32)
            x, y = pole.astype(np.float64) - a, target.astype(np.float64) - a
            angle = np.arccos(np.clip(x @ y / np.linalg.norm(x) / np.linalg.norm(y), -1, 1))
            if 0.2 <= angle <= np.pi - 0.2 and np.linalg.norm(x) > 0.2:
                break
        out.append(dict(tag=f"random {it}", parent=parent, locals=l, cons=[IM.two_bone(3, use_pole)], goals=[IM.goal(target, 1.0, pole)], bind=None))
    return out


def tip_in_frame(locals_, root, mid, tip):
    """float64: the tip of the chain in the frame of the root's parent"""
    W = IM.world64(np.array([-1, 0, 1]), np.asarray(locals_, np.float64)[[root, mid, tip]])
    return W[2][:, 3]


def frames(case):
    """(P32, P64) of the chain of constraint 0: the world matrix of the root's parent as the binary32 levels leave it, and in float64"""
    parent = np.asarray(case["parent"], np.int64)
    tip = case["cons"][0]["joint"]
    above = parent[parent[parent[tip]]]
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    if above < 0:
        return ident, ident
    return RM.world(parent, case["locals"])[above].astype(np.float64), IM.world64(parent, case["locals"])[above]


def tip_tolerance(case, E0, E1, geo, c_F):
    P32, P64 = frames(case)
    turned = np.linalg.norm(P32[:, :3], 2) * (4.0 * np.linalg.norm(E0) * (geo["l1"] + geo["l2"]) + 4.0 * np.linalg.norm(E1) * geo["l2"])
    return turned + np.linalg.norm(P64[:, :3] - P32[:, :3], 2) * np.linalg.norm(c_F) + np.linalg.norm(P64[:, 3] - P32[:, 3])
