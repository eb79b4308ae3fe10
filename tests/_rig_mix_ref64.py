"""include/pt_rig_mix.h's rule in float64, written apart from tests/_rig_mix_model.py (the quaternion product as one signed tensor contraction,
not the header's expanded expressions; the layers as weighted sums), and a bound on |binary32 result - this| that is derived, not fitted.  The
mixed locals and their entrywise bound go on into tests/_rig_ref64.py's records, which carry them through the normalisation, the hierarchy and N.

The inputs are the binary32 keys, masks, weights and, per layer, the binary32 (ka, kb, u) the host hands the kernel.  The decisions are the
binary32 model's (the sign of a blend's shorter arc, the negation of dq, e == 0 and e == 1): a reference that decided differently near a tie
would describe another, equally valid, pose.

THE BOUND (DESIGN.md 2.32 holds the same derivation).  u = 2^-24, first order in u; E_x is the entrywise bound of x; the factor 1.01 that
_rig_ref64.records applies at the end covers the second order.
  Step 2.  u == 0: S is a key, E_S = 0.  Otherwise _rig_ref64.blend: E_S = 3u (|v a| + |u b|).
  Step 3.  e = weight * mask is one rounded product of exact inputs: E_e = u e; without a mask E_e = 0.
  Step 5.  acc' = v acc + e' S with v = fl(1 - e): v errs by E_e + u v.  v acc errs by v E_acc + |acc| (E_e + u v) + u |v acc|, e' S by
    e E_S + |S| E_e + u |e S|, the sum rounds once more, u (|v acc| + |e S|):
        E_acc' = v E_acc + e E_S + (|acc| + |S|) E_e + 3u (|v acc| + |e S|)
    e == 0 keeps acc and E_acc; e == 1 takes S and E_S.
  Step 6, t and s.  d = fl(S - R), R exact: E_d = E_S + u |d|.  p = fl(e d): E_p = e E_d + |d| E_e + u |e d|.  acc' = fl(acc + p):
        E_acc' = E_acc + E_p + u |acc'|
  Step 6, q.  A component of p (x) q is four products and three sums, c = sum_i +-p_a(i) q_b(i):
        E_c = sum_i (E_p[a] |q_b| + |p_a| E_q[b]) + 4u sum_i |p_a q_b|
    dq = S.q (x) conj(R.q) with E_q = 0 (R exact; conj and the negation are exact).  dq'_xyz = fl(e dq): e E_dq + |dq| E_e + u |e dq|.
    dq'_w = fl(v + fl(e dq_w)): (E_e + u v) + (e E_dq + |dq_w| E_e + u |e dq_w|) + u |dq'_w|.  acc.q' = dq' (x) acc.q by the line above.
  Step 7.  The paddings are 0 exactly.
  Then include/pt_rig.h step 1 (e_q = 3 E_q / |q| + 4u, _rig_ref64.records with e_loc) and what follows it there."""
import numpy as np

import _rig_mix_model as MM
import _rig_model as RM
import _rig_ref64 as R64

U, TINY = R64.U, R64.TINY

# p (x) q = sum_ab QT[c, a, b] p_a q_b on (x y z w)
QT = np.zeros((4, 4, 4))
for c, terms in enumerate([((3, 0, 1), (0, 3, 1), (1, 2, 1), (2, 1, -1)), ((3, 1, 1), (0, 2, -1), (1, 3, 1), (2, 0, 1)), ((3, 2, 1), (0, 1, 1), (1, 0, -1), (2, 3, 1)),
                           ((3, 3, 1), (0, 0, -1), (1, 1, -1), (2, 2, -1))]):
    for a, b, sign in terms:
        QT[c, a, b] = sign
QA = np.abs(QT)


def qmul(p, Ep, q, Eq):
    """(p (x) q, its entrywise bound) for (n, 4) arrays known to Ep and Eq"""
    out = np.einsum("cab,na,nb->nc", QT, p, q)
    E = np.einsum("cab,na,nb->nc", QA, Ep, np.abs(q)) + np.einsum("cab,na,nb->nc", QA, np.abs(p), Eq) + 4.0 * U * np.einsum("cab,na,nb->nc", QA, np.abs(p), np.abs(q))
    return out, E


def mix_locals(clips, masks, layers, n, mutate=None):
    """(locals (n, 12) float64, their entrywise bound E (n, 12)).  mutate: None, "side" (the additive delta composed on the other side, acc.q (x)
    dq') or "mask" (the mask ignored): the locals are then what a wrong implementation would compute, under the rule's own bound"""
    trace = []
    MM.mix_locals(clips, masks, layers, n, trace=trace)                  # the binary32 decisions
    acc = E = None
    for l, (y, seen) in enumerate(zip(layers, trace)):
        times, values = clips[y["clip"]]
        V = np.asarray(values, np.float32).reshape(len(times), n, 12)
        if seen["u"] == 0:
            S, ES = V[seen["ka"]].astype(np.float64), np.zeros((n, 12))
        else:
            S, ES = R64.blend(V[seen["ka"]], V[seen["kb"]], seen["u"], seen["key_flip"])
        if l == 0:
            acc, E = S.copy(), ES.copy()
            continue
        w = float(y["weight"])
        masked = y["mask"] >= 0 and mutate != "mask"
        e = w * np.asarray(masks[y["mask"]], np.float32).astype(np.float64) if masked else np.full(n, w)
        Ee = (U * e if masked else np.zeros(n))[:, None]
        e32 = seen["e"] if mutate != "mask" else e.astype(np.float32)   # (the decisions e == 0 and e == 1 follow the weight the reference uses)
        ec, v = e[:, None], (1.0 - e)[:, None]
        if y["mode"] == MM.OVERRIDE:
            sign = np.ones((n, 12))
            sign[:, 4:8] = np.where(seen["flip"], -1.0, 1.0)[:, None]
            new = v * acc + ec * sign * S
            En = v * E + ec * ES + (np.abs(acc) + np.abs(S)) * Ee + 3.0 * U * (np.abs(v * acc) + np.abs(ec * S))
            one = (e32 == 1)[:, None]
            new, En = np.where(one, S, new), np.where(one, ES, En)
        else:
            R = V[0].astype(np.float64)
            d = S - R
            Ed = ES + U * np.abs(d)
            new = acc + ec * d
            En = E + (ec * Ed + np.abs(d) * Ee + U * np.abs(ec * d)) + U * np.abs(new)
            conj = np.concatenate([-R[:, 4:7], R[:, 7:8]], axis=1)
            dq, Edq = qmul(S[:, 4:8], ES[:, 4:8], conj, np.zeros((n, 4)))
            dq = np.where(seen["neg"][:, None], -dq, dq)
            dp = ec * dq
            Edp = ec * Edq + np.abs(dq) * Ee + U * np.abs(dp)
            dp[:, 3] = v[:, 0] + dp[:, 3]
            Edp[:, 3] = Edp[:, 3] + (Ee[:, 0] + U * v[:, 0]) + U * np.abs(dp[:, 3])
            if mutate == "side":
                new[:, 4:8] = qmul(acc[:, 4:8], E[:, 4:8], dp, Edp)[0]
                En[:, 4:8] = qmul(dp, Edp, acc[:, 4:8], E[:, 4:8])[1]
            else:
                new[:, 4:8], En[:, 4:8] = qmul(dp, Edp, acc[:, 4:8], E[:, 4:8])
        keep = (e32 == 0)[:, None]
        acc, E = np.where(keep, acc, new), np.where(keep, E, En)
    for pad in (3, 11):
        acc[:, pad], E[:, pad] = 0.0, 0.0
    return acc, E + TINY * (E > 0)


def records(parent, clips, masks, layers, inv_bind=None, mutate=None):
    """(records (n, 24) float64, bound (n, 24)) of the mix: _rig_ref64.records over the mixed locals and their bound"""
    n = np.asarray(parent).size
    l64, E = mix_locals(clips, masks, layers, n, mutate=mutate)
    return R64.records(parent, l64, inv_bind, e_loc=E)
