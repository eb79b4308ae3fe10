"""include/pt_rig.h's rule in float64, written apart from tests/_rig_model.py (4 x 4 homogeneous matrices under @, the rotation as
I + 2 w [v]x + 2 [v]x^2 of the normalised quaternion, N as the transpose of numpy's inverse — not the header's expanded expressions), and a
bound on |binary32 result - this| that is derived, not fitted.

The inputs are the binary32 locals, inverse binds and parents.  The sign flip of a clip's blend is the binary32 model's: it is a decision, and a
reference that decided differently near a tie would describe another (equally valid) pose.  A clip's u is the binary32 u: the host computes it
and hands it to the kernel as an input.

THE BOUND (DESIGN.md 2.31 holds the same derivation).  u = 2^-24, first order in u; the factor 1.01 at the end covers the second order (the
first-order terms stay below 1e-3 relative at depth 256).  Entrywise bounds carried through a product of rotations grow like sqrt(3)^depth (the
absolute values of a rotation have norm up to sqrt(3)) and say nothing at depth 65; the 2-norm is what a rotation keeps.  So the error of a
matrix A is carried as e_A[i], a bound on the 2-norm of the error of row i of its linear part, and E_A[i], a bound on the error of its
translation entry i.  |a_i| is the 2-norm of row i, |A|_2 and |A|_F the spectral and the Frobenius norm of the linear part.
  Step 1.  The input q carries E_q per component (0 for given locals, the blend's below for a clip) and has length |q|.  n^2 is four products
    and three sums of non-negative values: relative 4u; n: relative 2u + u; a component q_i / n: relative 4u, absolute <= 4u, plus what E_q
    does: E_q / |q| directly and |q_i| * |q|_1 E_q / |q|^2 <= 2 E_q / |q| through n.  e_q = 3 E_q / |q| + 4u.
    An entry of R (tests/_skin_dq_ref64.py, step 3): e_R = 6 e_q + 5u.  l_ic = r_ic * s_c carries |s_c| (e_R + u) + E_s[c], so
    e_L[i] = |(|s_c| (e_R + u) + E_s[c])_c|_2 for every row; l_i3 = t_i is a copy: E_L[i] = E_t[i].
  Step 2.  A root: W = L and its error is L's.  A child, C = A o B (A = W_p, B = L): row i of C's linear part is a_i B.  Its error is the error of
    a_i times B, a_i times the error of B, and the rounding of three products and two sums per entry, entrywise <= 3u (|a_i| |B|)_k:
        e_C[i] = e_A[i] |B|_2 + |a_i| |dB|_F + 3u |a_i| |B|_F                     |dB|_F = |e_B|_2, the rows' bounds together
    and the translation entry, three products and three sums, the last one with a_i3:
        E_C[i] = e_A[i] |b_t| + |a_i| |E_B|_2 + E_A[i] + 4u (|a_i| |b_t| + |a_i3|)
    So each level adds (30u from its local matrix + 3u from the product) times the norms of the running product, |a_i| and |B|, and a chain
    of depth d carries d times that: the recursion below is that sum, level by level, with the norms that occur.
  Step 3.  M = W o B, B exact: the same two lines with e_B = E_B = 0.
  Step 4.  Every entry of row i of M's linear part is known to E_ik = e_M[i].  c = m_a m_b - m_c m_d: E_c = E_a |m_b| + |m_a| E_b + E_c' |m_d| + |m_c| E_d + 2u (|m_a m_b| + |m_c m_d|).
    det = (m00 c00 + m01 c01) + m02 c02: E_det = sum_k (E_M[0, k] |c_0k| + |m_0k| E_c[0, k]) + 3u sum_k |m_0k c_0k|.
    n = c / det.  The computed determinant lies at least low = |det| - E_det from zero, so the quotient of the computed values is within
    E_c / low + |c| E_det / (|det| low) of c / det (no expansion of 1 / det: this holds for every E_det < |det|), and the division rounds once:
    E_n = that + u (|n| + that).  A joint with E_det > |det| / 2 has no bound for N (a singular M).
  Step 5.  v = 1 - u rounds once (relative u); v a and u b round once each, their sum once: E = 3u (|v a| + |u b|) per component of t, q and s.
  tiny = 2^-126 covers roundings of denormal intermediates."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126


def _cross(v):
    z = np.zeros(v.shape[0])
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], axis=1), np.stack([v[:, 2], z, -v[:, 0]], axis=1), np.stack([-v[:, 1], v[:, 0], z], axis=1)], axis=1)


def local_matrices(locals_):
    """(n, 4, 4) float64, from binary32 locals or from a blend's float64 ones as they are"""
    l = np.asarray(locals_).reshape(-1, 12).astype(np.float64)
    n = l.shape[0]
    q = l[:, 4:8] / np.linalg.norm(l[:, 4:8], axis=1)[:, None]
    K = _cross(q[:, 0:3])
    R = np.eye(3)[None] + 2.0 * q[:, 3, None, None] * K + 2.0 * (K @ K)
    L = np.tile(np.eye(4), (n, 1, 1))
    L[:, :3, :3] = R * l[:, None, 8:11]
    L[:, :3, 3] = l[:, 0:3]
    return L


def blend(a, b, u, flips):
    """step 5 in float64 from the binary32 keys and the binary32 u: (locals (n, 12) float64, their entrywise error bound E (n, 12))"""
    a = np.asarray(a, np.float32).reshape(-1, 12).astype(np.float64)
    b = np.asarray(b, np.float32).reshape(-1, 12).astype(np.float64)
    u = float(np.float32(u))
    w = np.full(a.shape, u)
    w[:, 4:8] = np.where(np.asarray(flips, bool)[:, None], -u, u)
    out = (1.0 - u) * a + w * b
    E = 3.0 * U * (np.abs((1.0 - u) * a) + np.abs(w * b))
    for pad in (3, 11):
        out[:, pad], E[:, pad] = 0.0, 0.0
    return out, E


def records(parent, locals_, inv_bind=None, e_loc=None, mutate=None):
    """(records (n, 24) float64, bound (n, 24)): bound is 0 for the padding, inf for N where M is too close to singular.  locals_ may be float64
    (a blend's); e_loc: its entrywise error (n, 12), None: exact inputs.  mutate: None, "side" (the child composed on the wrong side) or
    "transpose" (N without the transpose): the records are then what a wrong implementation would compute, under the rule's own bound, for the
    test that shows the bound notices"""
    parent = np.asarray(parent, np.int64)
    n = parent.size
    l = np.asarray(locals_).reshape(n, 12).astype(np.float64)
    E_in = np.zeros((n, 12)) if e_loc is None else np.asarray(e_loc, np.float64).reshape(n, 12)
    L = local_matrices(l)
    nq = np.linalg.norm(l[:, 4:8], axis=1)
    e_q = 3.0 * E_in[:, 4:8].max(axis=1) / nq + 4.0 * U
    e_R = 6.0 * e_q + 5.0 * U
    EL = np.zeros((n, 3, 4))
    EL[:, :, :3] = (np.abs(l[:, 8:11]) * (e_R + U)[:, None] + E_in[:, 8:11])[:, None, :]
    EL[:, :, 3] = E_in[:, 0:3]
    W, Wm = np.zeros((n, 4, 4)), np.zeros((n, 4, 4))                  # the rule's, which the bound is of, and the (possibly mutated) answer

    def composed(A, eA, EtA, B, eB, EtB):
        """(e, Et) of fl(A o B): A (4 x 4) known to the row bounds eA (3,) and the translation bounds EtA (3,), B likewise"""
        rows = np.linalg.norm(A[:3, :3], axis=1)
        bt = np.linalg.norm(B[:3, 3])
        e = eA * np.linalg.norm(B[:3, :3], 2) + rows * np.linalg.norm(eB) + 3.0 * U * rows * np.linalg.norm(B[:3, :3])
        Et = eA * bt + rows * np.linalg.norm(EtB) + EtA + 4.0 * U * (rows * bt + np.abs(A[:3, 3]))
        return e, Et

    eL, EtL = np.linalg.norm(EL[:, :, :3], axis=2), EL[:, :, 3]
    eW, EtW = np.zeros((n, 3)), np.zeros((n, 3))
    for j in range(n):
        p = parent[j]
        if p < 0:
            W[j], Wm[j], eW[j], EtW[j] = L[j], L[j], eL[j], EtL[j]
        else:
            W[j], Wm[j] = W[p] @ L[j], (L[j] @ Wm[p] if mutate == "side" else Wm[p] @ L[j])
            eW[j], EtW[j] = composed(W[p], eW[p], EtW[p], L[j], eL[j], EtL[j])
    M, Mm, eM, EtM = W, Wm, eW, EtW
    if inv_bind is not None and n:
        B = np.tile(np.eye(4), (n, 1, 1))
        B[:, :3, :] = np.asarray(inv_bind, np.float32).reshape(n, 3, 4).astype(np.float64)
        M, Mm = W @ B, Wm @ B
        both = [composed(W[j], eW[j], EtW[j], B[j], np.zeros(3), np.zeros(3)) for j in range(n)]
        eM, EtM = np.array([b[0] for b in both]), np.array([b[1] for b in both])
    EM = np.concatenate([np.repeat(eM[:, :, None], 3, axis=2), EtM[:, :, None]], axis=2)      # entrywise: an entry errs by at most its row
    out, bound = np.zeros((n, 24)), np.zeros((n, 24))
    if n == 0:
        return out, bound
    out[:, :12] = Mm[:, :3, :].reshape(n, 12)
    bound[:, :12] = (1.01 * EM + TINY).reshape(n, 12)
    A, EA = M[:, :3, :3], EM[:, :, :3]
    with np.errstate(all="ignore"):
        Am = Mm[:, :3, :3]
        inv = np.linalg.inv(np.where(np.abs(np.linalg.det(Am))[:, None, None] > 0, Am, np.eye(3)[None]))
        N = inv if mutate == "transpose" else np.transpose(inv, (0, 2, 1))
        c, Ec = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
        for i in range(3):
            for k in range(3):
                i1, i2, k1, k2 = (i + 1) % 3, (i + 2) % 3, (k + 1) % 3, (k + 2) % 3
                ma, mb, mc, md = A[:, i1, k1], A[:, i2, k2], A[:, i1, k2], A[:, i2, k1]
                c[:, i, k] = ma * mb - mc * md
                Ec[:, i, k] = (EA[:, i1, k1] * np.abs(mb) + np.abs(ma) * EA[:, i2, k2] + EA[:, i1, k2] * np.abs(md) + np.abs(mc) * EA[:, i2, k1]
                               + 2.0 * U * (np.abs(ma * mb) + np.abs(mc * md)))
        det = (A[:, 0, :] * c[:, 0, :]).sum(axis=1)
        Edet = (EA[:, 0, :] * np.abs(c[:, 0, :]) + np.abs(A[:, 0, :]) * Ec[:, 0, :]).sum(axis=1) + 3.0 * U * np.abs(A[:, 0, :] * c[:, 0, :]).sum(axis=1)
        low = np.abs(det) - Edet                                          # the computed determinant is at least this far from zero
        En = Ec / low[:, None, None] + np.abs(c) * (Edet / (np.abs(det) * low))[:, None, None]
        En = En + U * (np.abs(c / det[:, None, None]) + En)
        ok = Edet <= np.abs(det) / 2.0
        En = np.where(ok[:, None, None], 1.01 * En + TINY, np.inf)
    out[:, 12:21] = N.reshape(n, 9)
    bound[:, 12:21] = En.reshape(n, 9)
    return out, bound
