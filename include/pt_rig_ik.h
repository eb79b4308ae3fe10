/* include/pt_rig_ik.h — two-bone and aim constraints solved on the device: world-space goals turned into joint rotations where the rig's locals
 * lie, between a call's source and its levels (libpt_hip.so).
 *
 * No reference counterpart.  A rig of include/pt_rig.h plays locals, a clip or a mix of clips (include/pt_rig_mix.h).  A foot planted on a ramp, a
 * hand on a handle, a head that follows a light are goals in world space, and clips cannot say them: without this header the caller downloads or
 * re-makes the locals, walks the hierarchy on the host for the parent's world matrix, solves there and uploads n_parts * 48 bytes again on every
 * step.  Here the constraints are attached once, a step uploads 32 bytes per goal, and the solve runs where the world matrices already lie.
 *
 * OBJECTS.  A rig gains
 *   a CONSTRAINT TABLE (pt_rig_ik_attach): any number of pt_rig_ik_constraint, 32 bytes each.  An attach replaces the table (0 bytes: no table)
 *     and clears the goals; the rig changes only once the new table stands.
 *       PT_RIG_IK_TWO_BONE names the TIP in `joint`.  mid = parent[tip] and root = parent[mid] must both exist.  It writes the rotations of root
 *         and mid.  With PT_RIG_IK_POLE in flags the goal's pole is read.  axis is not read.
 *       PT_RIG_IK_AIM names one joint and a unit axis in that joint's own frame.  It writes that joint's rotation.  The pole is never read.
 *     The FIRST JOINT of a constraint is the root of a chain, or the aimed joint.  Translations, scales and padding are never written.
 *   GOALS (pt_rig_ik_goals): one pt_rig_ik_goal per constraint, in the table's order, in world space (the space the rig's W are in: what a root's
 *     local maps into).  They are state on the rig, like pt_morph_weights on a pose: while goals are set, every record call of the rig
 *     (pt_rig_records, pt_rig_clip_records, pt_rig_mix_records, pt_rig_pose_geometry, pt_rig_clip_pose_geometry, pt_rig_mix_pose_geometry) and
 *     pt_rig_ik_locals runs the rule below between its source and its levels.  (NULL, 0) sets them off again.
 *
 * INDEPENDENCE, checked at the attach on the host.  W(A) is the set of joints constraint A writes.  R(A) is the set it reads: its own joints
 * (root, mid and tip, or the aimed joint) and every ancestor of its first joint.  For constraints A != B, W(A) and R(B) must not meet.  Then the
 * constraints of a call are free of order.  Two arms, two legs and a head on one spine pass; an aim on a solved chain's tip, an aim on an
 * ancestor of a chain and two chains that share a mid do not.
 *
 * THE RULE.  Binary32 throughout, every product rounded before every sum, in the written order, nothing fused; sqrt and / correctly rounded, as
 * in include/pt_rig.h, whose LOCAL and steps are meant below, and include/pt_rig_mix.h, whose step 6 gives p (x) q.  Stated as: the levels of
 * include/pt_rig.h over the call's locals (a full pass), then every constraint on its own as below, then a full pass again over the changed
 * locals.  (The implementation runs only the levels either pass needs; the result is the same bits.)  For vectors of three,
 *      dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z        |a| = sqrt(dot(a, a))        cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)
 *      R(q) the nine expressions of include/pt_rig.h step 1 on q as it is (not normalised here);  R.v per row i: (r_i0*v.x + r_i1*v.y) + r_i2*v.z
 *      n(q): q normalised as in include/pt_rig.h step 1;  L = R(n(q)) with column c times s_c, as there;  L.v likewise
 *      ok(x): x != 0 and |x| <= FLT_MAX (no zero, no infinity, no NaN)
 * Everything happens in the frame F of the first joint's parent.
 *
 * 0. A goal of weight 0 leaves its constraint's joints as they are, bit for bit: nothing below is evaluated, the quaternions are not normalised.
 * 1. Goal and pole in F.  P is the world matrix of the first joint's parent after the first pass.  c_ik and det are include/pt_rig.h step 4's
 *    cofactors and determinant of P's linear part.  For x the target, and the pole when it is read:
 *      d_i = x_i - p_i3        x_F[k] = ((c_0k*d_0 + c_1k*d_1) + c_2k*d_2) / det
 *    A first joint that is a root of the rig takes x as it is, bit for bit, and det counts as ok.
 * 2. TWO_BONE, the chain in F.  n0 = n(q_root), n1 = n(q_mid), L0 and L1 their local matrices.
 *      a = t_root        b = L0.t_mid + a        c = L0.(L1.t_tip + t_mid) + a        (each sum per component, the matrix product first)
 *      e1 = b - a, l1 = |e1|        e2 = c - b, l2 = |e2|        v = g_F - a, dist = |v|, eh = v / dist
 * 3. The triangle.
 *      lo = |l1 - l2|, hi = l1 + l2;  d = dist < lo ? lo : dist;  d = d > hi ? hi : d
 *      cosA = ((l1*l1 + d*d) - l2*l2) / ((2*l1)*d);  cosA = cosA < -1 ? -1 : cosA;  cosA = cosA > 1 ? 1 : cosA;  sinA = sqrt(1 - cosA*cosA)
 *      h0 = pole_F - a with PT_RIG_IK_POLE, else e1;   h = h0 - eh*dot(h0, eh) per component;   hl = |h|, hh = h / hl
 *      u1 = cosA*eh + sinA*hh per component;   b' = a + l1*u1;   c' = a + d*eh
 * 4. The rotations.  fromTo(u, v) for unit u and v is the half-angle form, without an arccosine:
 *      m = u + v, ml = |m|, mh = m / ml, fromTo = (cross(u, mh), dot(u, mh))        as (x y z | w)
 *    When ml == 0 exactly (v == -u: antiparallel) the half turn about a fixed FALLBACK AXIS is taken: k = cross(u, X) with X = (1, 0, 0), that is
 *    (0, u.z, -u.y), and fromTo = (k / |k|, 0); when |k| == 0 too (u along X), fromTo = (0, 0, 1, 0), the half turn about Z.
 *      r1 = fromTo(e1 / l1, u1)        e2' = R(r1).e2, l2' = |e2'|        w = c' - b', wl = |w|        r2 = fromTo(e2' / l2', w / wl)
 *      q_root* = r1 (x) n0        q_mid* = ((conj(q_root*) (x) r2) (x) q_root*) (x) n1
 * 5. AIM on joint j.  nj = n(q_j), u = R(nj).axis, w = g_F - t_j, wl = |w|, q_j* = fromTo(u, w / wl) (x) nj.
 * 6. The weight.  Weight 1 stores q* bit for bit.  Any other weight e stores the shorter-arc lerp of include/pt_rig.h step 5 between n (the
 *    normalised quaternion the solve started from) and q*: v = 1 - e, d = ((n.x*q*.x + n.y*q*.y) + n.z*q*.z) + n.w*q*.w, e' = d < 0 ? -e : e, per
 *    component v*n + e'*q*.  It is not normalised; step 1 of include/pt_rig.h normalises later.
 * 7. Left as it is.  A constraint leaves its joints as they are, bit for bit, when the target holds a NaN or any of these is not ok:
 *      TWO_BONE: det, l1, l2, dist, hl, l2', wl        AIM: det, wl
 *    (an unreadable pole shows as hl, a target at the chain's root as dist, a target or pole on the line of the bend as hl.)
 * A NON-RIGID CHAIN — a non-uniform scale on root or mid, which the rotation then shears differently — gets whatever these expressions give: the
 * tip then misses the target.  A target beyond the reach gives the fully extended chain towards it (d = hi), one inside |l1 - l2| the folded one.
 *
 * CONTRACTS.
 *   pt_rig_ik_locals is the rule alone: the given locals uploaded, the first pass, the constraints, the locals downloaded.  With goals off it
 *   returns the locals as given.  Each of the six record calls, with goals set, equals pt_rig_records with goals off of what pt_rig_ik_locals
 *   returns for that call's source's locals, bit for bit.  pt_rig_mix_locals stays the mix alone.
 *   With no table, with goals off, or with every weight 0, every call answers bit for bit as it does without this header.
 *   A clip's keys are never written: a source that answers in place (a time at a key) is copied first.
 *
 * REFUSALS, all PT_ERR_ARG, in this order (the first failing check answers):
 *   pt_rig_ik_attach          a null or destroyed rig; bytes no multiple of 32; null constraints with bytes > 0; then per constraint, in the
 *                             order of the table: an unknown kind; a joint outside [0, n_parts); (TWO_BONE) a tip without a parent and a
 *                             grandparent; flags other than 0 or PT_RIG_IK_POLE; (AIM) an axis that is not finite or whose length is off 1 by
 *                             more than 1e-3; then constraints that are not independent.
 *   pt_rig_ik_goals           a null or destroyed rig; null goals with bytes > 0; (goals given) bytes != 32 * the table's constraints; a weight
 *                             that is not finite or lies outside [0, 1].
 *   pt_rig_ik_locals          a null or destroyed rig; null locals with n_parts > 0; local_bytes != n_parts * 48; null locals_out;
 *                             out_bytes != n_parts * 48.
 *
 * OWNERSHIP, ORDER and threads: as include/pt_rig.h; the table and the goals go with their rig.  pt_debug_rig_ik_time (include/pt_debug.h) times
 * the solve's launch.
 *
 * NOT BUILT: dependent constraints solved in passes (an aim on a solved chain's tip), chains of more than two bones, iterative solvers, joint
 * limits, a twist of the tip to a goal orientation, goals given in a joint's frame, rows sorted by kind (a wave that holds both kinds runs both).
 */
#ifndef PT_RIG_IK_H
#define PT_RIG_IK_H
#include "pt_rig.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PT_RIG_IK_TWO_BONE 0
#define PT_RIG_IK_AIM      1
#define PT_RIG_IK_POLE     1    /* flags bit 0: the goal's pole is read */

typedef struct pt_rig_ik_constraint {
    int32_t kind, joint, flags, pad;    /* PT_RIG_IK_TWO_BONE: joint is the tip; PT_RIG_IK_AIM: the aimed joint */
    float axis[3], padf;                /* AIM: the unit axis in the joint's own frame */
} pt_rig_ik_constraint;

typedef struct pt_rig_ik_goal {
    float target[3], weight;            /* world space; weight in [0, 1] */
    float pole[3], padf;                /* world space, read with PT_RIG_IK_POLE */
} pt_rig_ik_goal;

int pt_rig_ik_attach(pt_rig* rig, const pt_rig_ik_constraint* constraints, size_t bytes);
int pt_rig_ik_goals(pt_rig* rig, const pt_rig_ik_goal* goals, size_t bytes);
int pt_rig_ik_locals(pt_rig* rig, const float* locals, size_t local_bytes, float* locals_out, size_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif
