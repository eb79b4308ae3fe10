/* include/pt_skin_dq.h — dual-quaternion skinning of a scene's triangles, all on the device (libpt_hip.so).
 *
 * No reference counterpart.  include/pt_skin.h blends the MATRICES of up to four bones per corner.  Between two bones that are twisted against
 * each other that blend is no rotation and the surface shrinks: a corner weighted 0.5 / 0.5 between bones turned by theta about their common axis
 * lands at |cos(theta / 2)| of its distance from the axis — half the radius at 120 degrees, a point at 180 (the "candy wrapper").  A DQ POSE is a
 * pt_pose whose rule turns every bone's record into a unit dual quaternion, blends those per corner, normalises the blend and turns it back into
 * a rigid record: always a rotation plus a translation, so nothing shrinks.  It is created by pt_skin_dq_create and then used with
 * pt_pose_geometry, pt_pose_triangles, pt_pose_destroy, pt_morph_attach, pt_morph_weights, pt_normals_attach and pt_normals_mode exactly as a
 * skinned pose of pt_skin_create: the same n_parts records of 24 floats, the same two corner tables with the same layout and the same static-corner
 * rule (include/pt_skin.h, THE TABLES), the same contract (the state pt_move_geometry of the posed triangles would leave), the same staleness, slow
 * paths, behind / settle behaviour and ownership.  Only the rule differs.
 *
 * THE RULE.  Binary32 throughout, every product rounded before every sum, nothing fused, sqrt and / correctly rounded.
 *
 * 1. Record -> dual quaternion, once per record and pose, from floats 0-11 only (N and the padding are ignored).  With M's rows (m00 m01 m02 tx),
 *    (m10 m11 m12 ty), (m20 m21 m22 tz) and tr = (m00 + m11) + m22:
 *      tr > 0:                          s = sqrt(tr + 1) * 2,                   w = 0.25*s,       x = (m21 - m12)/s, y = (m02 - m20)/s, z = (m10 - m01)/s
 *      else m00 > m11 && m00 > m22:     s = sqrt(((1 + m00) - m11) - m22) * 2,  w = (m21 - m12)/s, x = 0.25*s,       y = (m01 + m10)/s, z = (m02 + m20)/s
 *      else m11 > m22:                  s = sqrt(((1 + m11) - m00) - m22) * 2,  w = (m02 - m20)/s, x = (m01 + m10)/s, y = 0.25*s,       z = (m12 + m21)/s
 *      else:                            s = sqrt(((1 + m22) - m00) - m11) * 2,  w = (m10 - m01)/s, x = (m02 + m20)/s, y = (m12 + m21)/s, z = 0.25*s
 *    then n = sqrt(((w*w + x*x) + y*y) + z*z) and w, x, y, z are each divided by n.  The dual part:
 *      dw = -0.5 * ((tx*x + ty*y) + tz*z)        dx = 0.5 * ((tx*w + ty*z) - tz*y)
 *      dy =  0.5 * ((ty*w + tz*x) - tx*z)        dz = 0.5 * ((tz*w + tx*y) - ty*x)
 *    8 floats per record, q = (w x y z)(dw dx dy dz).  The rotation part of M is the caller's to keep orthonormal; nothing checks it, and a
 *    record that is no rigid motion gives whatever these expressions give.
 * 2. The blend of a corner with n >= 1 slots, b_s and w_s its bone ids and weights.  Slot 0's real part is the pivot: for s >= 1,
 *      w'_s = -w_s  if (((q0.w*qs.w + q0.x*qs.x) + q0.y*qs.y) + q0.z*qs.z) < 0, else w_s         (the shorter arc; negating is exact)
 *      Br = w_0 * qr_0,  Br = Br + (w'_s * qr_s)   s = 1 .. n-1, in that order, per component; Bd likewise from the dual parts
 *      L = sqrt(((Br.w*Br.w + Br.x*Br.x) + Br.y*Br.y) + Br.z*Br.z),  r = Br / L,  d = Bd / L
 *    The weights of empty slots are never multiplied (they may be NaN).
 * 3. Back to a record B of 24 floats.  With r = (w x y z), xx = x*x and so on (a product with 2 is exact):
 *      row0 = (1 - 2*(yy + zz),   2*(xy - wz),       2*(xz + wy))
 *      row1 = (2*(xy + wz),       1 - 2*(xx + zz),   2*(yz - wx))
 *      row2 = (2*(xz - wy),       2*(yz + wx),       1 - 2*(xx + yy))
 *      t.x = 2*(((d.x*w - d.w*x) + d.z*y) - d.y*z)
 *      t.y = 2*(((d.y*w - d.w*y) + d.x*z) - d.z*x)
 *      t.z = 2*(((d.z*w - d.w*z) + d.y*x) - d.x*y)
 *    B's M is [R | t], its N is R, its padding is 0.
 * 4. include/pt_pose.h's rule with B in place of the part's record: the corner's vertex under B's M, its normal under B's N.
 *
 * CONSEQUENCES.
 *   1. A static corner (slot 0 holds -1) is the rest pose's, bit for bit, and no kernel ever writes it.
 *   2. Two corners with the same rest floats and the same 4 + 4 skin words get the same bits: a shared vertex does not crack.
 *   3. An identity record converts to (1 0 0 0)(0 0 0 0) exactly.  A corner all of whose bones hold the identity, with weights that sum to 1 in
 *      exact arithmetic (0.25 x 4, say), is posed by the exact identity B.
 *   4. Unlike the linear skin, the single-slot weight-1 DQ skin is NOT pt_pose_triangles' output bit for bit: matrix -> quaternion -> matrix
 *      rounds.  It is that pose within a bound derived from the operation count (tests/_skin_dq_ref64.py).
 *   5. A blend of zero length gives NaN: weights (1, -1) on one bone, say.  pt_pose_geometry refuses it as it refuses every NaN coordinate
 *      (PT_ERR_SCENE), and the last accepted pose is restored as for any refusal.
 *
 * REFUSALS of pt_skin_dq_create: the seven of pt_skin_create (include/pt_skin.h), in the same order and with the same texts, all PT_ERR_ARG under
 * the name pt_skin_dq_create; then whatever pt_pose_create returns after its argument checks.  pt_debug_pose_time and pt_debug_skin_time
 * (include/pt_debug.h) refuse a DQ pose with PT_ERR_ARG; pt_debug_skin_dq_time times its two kernels and refuses every other pose.
 *
 * NOT BUILT: more than four slots; 16-bit packed tables; a choice between the linear and the dual-quaternion blend per corner of one skin; scale
 * or shear carried beside the dual quaternion; posed ellipsoids; JNI natives; rebuilding degraded trees.
 */
#ifndef PT_SKIN_DQ_H
#define PT_SKIN_DQ_H
#include "pt_skin.h"
#ifdef __cplusplus
extern "C" {
#endif

int pt_skin_dq_create(pt_ctx* ctx,
                      const int32_t* corner_bone, size_t bone_bytes,      /* as for pt_skin_create */
                      const float* corner_weight, size_t weight_bytes,
                      int n_parts, pt_pose** out);

#ifdef __cplusplus
}
#endif
#endif
