"""include/pt_skin_dq.h's rule in float64, written apart from tests/_skin_dq_model.py (quaternion products: the dual part as 0.5 (0, t) q, the
translation as the vector part of 2 d q*, the rotation as the sandwich q v q*, not the header's expanded expressions), and a bound on
|binary32 result - this| that is derived, not fitted.

The inputs are the binary32 records, tables and rest pose.  The conversion's branch per record and the sign flip per slot are the binary32
model's: both are decisions, and a reference that decided differently near a tie would describe another (equally valid) pose.

The bound.  u = 2^-24.  u_in is the error the record's floats carry against the rigid motion they stand for: 0 when the binary32 model is
compared with this evaluation of the SAME floats, u when it is compared with the geometry that a record rounded once from binary64 means
(rotation entries: absolute error <= u since |m| <= 1; translation: relative error u).  First order in u; the factor 1.01 at the end covers the
second order (every first-order term below is < 3000 u = 2e-4 relative for L >= FLOOR, far inside 1 %).  T = |t|_2 of a record.
  Step 1.  tr = (m00 + m11) + m22: two roundings of values <= 2 and <= 3, 3 u_in from the inputs.  p = tr + 1 resp. ((1 + mii) - mjj) - mkk:
    |error| <= 9u + 3 u_in, and p >= 1: of w^2 .. z^2, which sum to 1, branch 0 is taken when w^2 = (1 + tr) / 4 > 1/4, and otherwise the largest of
    x^2, y^2, z^2 (the order of the diagonal is their order) is >= (1 - 1/4) / 3.  So s = 2 sqrt(p) >= 2 with relative error 5.5u + 1.5 u_in, the
    component 0.25 s has absolute error <= 5.5u + 1.5 u_in, and a component (a +- b) / s: (2u + 2 u_in) / s from the numerator, its own size (<= 1) times
    s's relative error, one rounding: <= 7.5u + 2.5 u_in = e1.  n^2 = ((ww + xx) + yy) + zz: 2 (|w| + .. + |z|) e1 <= 4 e1 from the components, four
    products and three sums of values <= 1: 4u; n relative 2 e1 + 2u + u; a normalised component: e_q = e1 + (2 e1 + 3u) + u = 3 e1 + 4u.
    A dual component, 0.5 * (three products t_i q_j, two sums): sqrt(3) T e_q from q (|t|_1 <= sqrt(3) T), u_in T from t, u T from the three
    products (Cauchy-Schwarz, |q| <= 1) and 2u T from the sums: e_dual = 0.5 T (sqrt(3) e_q + u_in + 3u).  |dual| <= T / 2.
  Step 2.  W = sum |w_s| over the used slots, Tm = the largest T among them.  A component of Br: W e_q from the table, u W from the products,
    at most three sums of partial values <= W: e_Br = W (e_q + 4u).  Of Bd alike: e_Bd = W (0.5 Tm (sqrt(3) e_q + u_in + 3u) + 2u Tm).
    L^2: 2 |Br|_1 e_Br <= 4 L e_Br and 4u L^2; L relative 2 e_Br / L + 3u.  r = Br / L: e_r = 3 e_Br / L + 4u per component.  d = Bd / L with
    D = |Bd|_2 / L: e_d = e_Bd / L + D (2 e_Br / L + 4u) per component.  L is the reference's; a corner with L < FLOOR has no bound.
  Step 3.  A diagonal entry 1 - 2 (yy + zz): 4 (|y| + |z|) e_r <= 4 sqrt(2) e_r, the products and their sum 4u, the last difference u.  An
    off-diagonal one, 2 (xy -+ wz): 2 (|w| + |x| + |y| + |z|) e_r <= 4 e_r and 2u.  Both <= e_R = 6 e_r + 5u.
    t: 2 * (four products d_i r_j, three sums): 2 |d|_1 e_r <= 4 D e_r... in all e_t = 4 D e_r + 4 e_d + 8u D.
  Step 4.  A vertex float ((R0 x + R1 y) + R2 z) + t: |v|_1 e_R + e_t, three products and two sums of values <= |v|_2, the last sum of a value
    <= |v|_2 + |t_B|: e_v = |v|_1 e_R + e_t + u (4 |v|_2 + |t_B|_2).  A normal float: e_n = |n|_1 e_R + 3u |n|_2.
  tiny = 2^-126 covers roundings of denormal intermediates."""
import numpy as np

U = 2.0 ** -24
FLOOR = 0.25                 # blends with L below this are excluded from the bound (the error grows like 1 / L)
SQRT3 = 3.0 ** 0.5


def qmul(a, b):
    """Hamilton product of (n, 4) arrays, (w x y z)"""
    aw, ax, ay, az = (a[:, j] for j in range(4))
    bw, bx, by, bz = (b[:, j] for j in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=1)


def conj(a):
    return a * np.array([1.0, -1.0, -1.0, -1.0])


def dq_from_records(xforms, branch):
    """(real (n, 4), dual (n, 4), T (n,)) in float64, by the branch the binary32 model took"""
    X = np.asarray(xforms, np.float32).reshape(-1, 24).astype(np.float64)
    n = X.shape[0]
    M = X[:, :12].reshape(n, 3, 4)
    q = np.zeros((n, 4))
    for k in range(n):
        m, b = M[k, :, :3], int(branch[k])
        if b == 0:
            s = np.sqrt(m[0, 0] + m[1, 1] + m[2, 2] + 1.0) * 2.0
            q[k] = (0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s)
        else:
            i = b - 1
            j, l = (i + 1) % 3, (i + 2) % 3
            s = np.sqrt(1.0 + m[i, i] - m[j, j] - m[l, l]) * 2.0
            q[k, 0] = (m[l, j] - m[j, l]) / s
            q[k, 1 + i] = 0.25 * s
            q[k, 1 + j] = (m[i, j] + m[j, i]) / s
            q[k, 1 + l] = (m[i, l] + m[l, i]) / s
    q /= np.linalg.norm(q, axis=1)[:, None]
    t = np.concatenate([np.zeros((n, 1)), M[:, :, 3]], axis=1)
    return q, 0.5 * qmul(t, q), np.linalg.norm(M[:, :, 3], axis=1)


def skin_dq(rest, bone, weight, xforms, branch, flips, u_in=0.0):
    """(out (n_tris, 40) float64, bound (n_tris, 40), L (3 n_tris,)): bound is 0 for the floats the rule copies and inf for corners with L < FLOOR"""
    rest = np.asarray(rest, np.float32).reshape(-1, 40).astype(np.float64)
    n = rest.shape[0]
    bone = np.asarray(bone, np.int64).reshape(-1, 4)
    w = np.asarray(weight, np.float32).reshape(-1, 4).astype(np.float64)
    flips = np.asarray(flips, bool).reshape(-1, 4)
    qr, qd, T = dq_from_records(xforms, branch)
    used = np.cumprod(bone >= 0, axis=1).astype(bool)
    moving = np.nonzero(used[:, 0])[0]
    out, bound, Ls = rest.copy(), np.zeros((n, 40)), np.full(3 * n, np.inf)
    if moving.size == 0:
        return out, bound, Ls
    b, u = np.where(used, bone, 0)[moving], used[moving]
    ws = np.where(u, np.where(flips[moving], -w[moving], w[moving]), 0.0)
    Br = np.einsum("cs,csj->cj", ws, qr[b])
    Bd = np.einsum("cs,csj->cj", ws, qd[b])
    L = np.linalg.norm(Br, axis=1)
    with np.errstate(all="ignore"):
        r, d = Br / L[:, None], Bd / L[:, None]
        tB = 2.0 * qmul(d, conj(r))[:, 1:]
        k, c = moving // 3, moving % 3
        v = np.stack([rest[k, 4 * c + j] for j in range(3)], axis=1)
        nr = np.stack([rest[k, 12 + 4 * c + j] for j in range(3)], axis=1)
        zero = np.zeros((moving.size, 1))
        pv = qmul(qmul(r, np.concatenate([zero, v], axis=1)), conj(r))[:, 1:] + tB
        pn = qmul(qmul(r, np.concatenate([zero, nr], axis=1)), conj(r))[:, 1:]
        # the bound
        W = np.abs(ws).sum(axis=1)
        Tm = np.where(u, T[b], 0.0).max(axis=1)
        e1 = 7.5 * U + 2.5 * u_in
        eq = 3.0 * e1 + 4.0 * U
        eBr = W * (eq + 4.0 * U)
        eBd = W * (0.5 * Tm * (SQRT3 * eq + u_in + 3.0 * U) + 2.0 * U * Tm)
        D = np.linalg.norm(Bd, axis=1) / L
        er = 3.0 * eBr / L + 4.0 * U
        ed = eBd / L + D * (2.0 * eBr / L + 4.0 * U)
        eR = 6.0 * er + 5.0 * U
        et = 4.0 * D * er + 4.0 * ed + 8.0 * U * D
        ev = np.abs(v).sum(axis=1) * eR + et + U * (4.0 * np.linalg.norm(v, axis=1) + np.linalg.norm(tB, axis=1))
        en = np.abs(nr).sum(axis=1) * eR + 3.0 * U * np.linalg.norm(nr, axis=1)
        ev = np.where(L >= FLOOR, 1.01 * ev + 2.0 ** -126, np.inf)
        en = np.where(L >= FLOOR, 1.01 * en + 2.0 ** -126, np.inf)
    for j in range(3):
        out[k, 4 * c + j], out[k, 12 + 4 * c + j] = pv[:, j], pn[:, j]
        bound[k, 4 * c + j], bound[k, 12 + 4 * c + j] = ev, en
    Ls[moving] = L
    return out, bound, Ls


def corner_rotations(bone, weight, xforms, branch, flips):
    """the blended rotation matrices (n_corners, 3, 3) and translations (n_corners, 3) of the moving corners in float64 (static ones: NaN)"""
    bone = np.asarray(bone, np.int64).reshape(-1, 4)
    m = bone.shape[0]
    # one triangle per corner, its three corners under that corner's words: the zero vertex lands on t, the normals e_x, e_y, e_z on R's columns
    rest = np.zeros((m, 40))
    for c in range(3):
        rest[:, 12 + 4 * c + c] = 1.0
    rep = lambda a: np.repeat(a.reshape(m, 1, 4), 3, axis=1).reshape(-1)
    o, _, _ = skin_dq(rest, rep(bone), rep(np.asarray(weight, np.float32)), xforms, branch, rep(np.asarray(flips, bool)))
    R = np.stack([o[:, 12 + 4 * c:15 + 4 * c] for c in range(3)], axis=2)
    t = o[:, 0:3].copy()
    R[bone[:, 0] < 0] = np.nan
    t[bone[:, 0] < 0] = np.nan
    return R, t
