/* include/pt_rig.h — a joint hierarchy and keyed clips evaluated on the device: the records of a pose made where they are used (libpt_hip.so).
 *
 * No reference counterpart.  include/pt_pose.h and its rules take n_parts records of 24 floats; making them was the caller's work: walk the
 * skeleton, multiply in the inverse bind matrices, invert and transpose for N, interpolate between keys, on the host and on every step.  A RIG
 * is attached to a pose object of any of the three rules (pt_pose_create, pt_skin_create, pt_skin_dq_create; morph and normals attached or not)
 * and does that on the device: it turns local joint transforms, or a time into a keyed clip, into that pose's records, and hands them to the
 * pose's rule where they lie.  A step of a baked animation uploads one float.
 *
 * A RIG (pt_rig_create) has one joint per record of its pose: joint j writes record j, n_joints == n_parts.  parent[j] lies in [-1, j): parents
 * come before their children, -1 marks a root, several roots are allowed.  inv_bind, when given, holds one 3 x 4 row-major matrix B_j per joint
 * (12 floats, rows (b_i0 b_i1 b_i2 b_i3)).  The DEPTH of a rig is the number of joints on its longest chain from a root (a root alone: 1); it
 * may not exceed PT_RIG_MAX_DEPTH.  A pose may have several rigs.
 *
 * A LOCAL is 12 floats per joint:  t.x t.y t.z pad | q.x q.y q.z q.w | s.x s.y s.z pad  — translation, rotation quaternion, scale; the two
 * padding floats are never read.
 *
 * THE RULE.  Binary32 throughout, every product rounded before every sum, in the written order, nothing fused; sqrt and / correctly rounded
 * (the conventions of include/pt_skin_dq.h).  A 3 x 4 matrix A has the linear part a_ik, k = 0..2, and the translation a_i3.
 *
 * 1. Local matrix L_j.  n = sqrt(((x*x + y*y) + z*z) + w*w) and x, y, z, w are each divided by n.  R from (w x y z) by the expressions of
 *    include/pt_skin_dq.h step 3:
 *      row0 = (1 - 2*(yy + zz),   2*(xy - wz),       2*(xz + wy))
 *      row1 = (2*(xy + wz),       1 - 2*(xx + zz),   2*(yz - wx))
 *      row2 = (2*(xz - wy),       2*(yz + wx),       1 - 2*(xx + yy))
 *    l_ic = r_ic * s_c (c = 0, 1, 2: column c is scaled by component c of s), l_i3 = t_i.
 * 2. World matrix W_j.  A root has W_j = L_j, bit for bit: nothing is multiplied by an identity.  Otherwise W_j = W_parent o L_j with
 *      (A o B)_ik = ((a_i0*b_0k + a_i1*b_1k) + a_i2*b_2k)                    k = 0, 1, 2
 *      (A o B)_i3 = (((a_i0*b_03 + a_i1*b_13) + a_i2*b_23) + a_i3)
 *    The association is fixed, root first: ((L_root o ...) o L_parent) o L_j.
 * 3. Record M.  M_j = W_j o B_j; with inv_bind == NULL, M_j = W_j bit for bit.  M is floats 0-11 of record j.
 * 4. Record N, floats 12-20: the cofactor matrix of M's linear part over its determinant (the inverse transpose).  With indices mod 3,
 *      c_ik = m_(i+1)(k+1) * m_(i+2)(k+2) - m_(i+1)(k+2) * m_(i+2)(k+1)        (c_00 = m11*m22 - m12*m21, and so on cyclically)
 *      det  = (m00*c_00 + m01*c_01) + m02*c_02
 *      n_ik = c_ik / det
 *    Floats 21-23 are 0.  A ZERO DETERMINANT (a zero scale, say) gives whatever these expressions give: infinities and NaNs in N.  Nothing
 *    checks it here; a pose whose normals meet them hands on what include/pt_pose.h's rule makes of them.
 * 5. Clip sampling (pt_rig_clip_attach).  A clip has n_keys >= 1 key times T_0 < T_1 < ..., finite, and n_keys * n_parts locals, key-major
 *    (key k's joint j at 12 * (k * n_parts + j)); it is copied to the device at the attach, and a second attach replaces the first.  A time t is
 *    clamped to [T_0, T_last] on the host; k is the interval with T_k <= t < T_k+1 (the last interval at t == T_last; with one key there is no
 *    interval and key 0 is taken); u = (t - T_k) / (T_k+1 - T_k) in binary32.  u == 0 takes key k bit for bit, u == 1 key k+1 bit for bit.
 *    Otherwise with a and b the locals of keys k and k+1, per joint, v = 1 - u:
 *      t and s, per component:   v*a + u*b
 *      q:  d = ((a.x*b.x + a.y*b.y) + a.z*b.z) + a.w*b.w,   u' = d < 0 ? -u : u,   per component v*a + u'*b      (the shorter arc; negating is exact)
 *    and step 1 normalises afterwards.  This is a NORMALISED LERP, NOT A SLERP: no transcendental function enters the rule, so the device and
 *    the CPU statement (csrc/hip/pt_rig_rule.hpp) agree bit for bit.  Against the slerp it runs at most a few per cent off the constant angular
 *    speed between two keys; a caller who needs better places more keys.
 * A NaN local reaches the pose as a NaN coordinate, and the pose refuses it (PT_ERR_SCENE) as it refuses every NaN.
 *
 * CONTRACTS.
 *   pt_rig_records / pt_rig_clip_records are the rule alone, downloaded: n_parts records of 24 floats.  They change nothing of the pose or the
 *   context.
 *   pt_rig_pose_geometry(ctx, rig, locals, ...) leaves the context, the pose and what a later settle delivers exactly as
 *   pt_pose_geometry(ctx, pose, R, ...) would with R what pt_rig_records returns: return codes, refusals and slow paths, in_place and root_cost,
 *   the image history, the last accepted state and its rerun after a refusal.  pt_rig_clip_pose_geometry does likewise with pt_rig_clip_records.
 *   On the in-place path no record is uploaded: the call uploads the locals (nothing for a clip) and downloads R, 96 bytes per part, which the
 *   pose keeps as its last accepted state and the slow paths start from.
 *
 * REFUSALS, all PT_ERR_ARG, in this order:
 *   pt_rig_create             null pose, parent or out; a pose that is not live (destroyed); parent_bytes != n_parts * 4;
 *                             a parent outside [-1, j); inv_bind given with bind_bytes != n_parts * 48; a depth above PT_RIG_MAX_DEPTH.
 *   pt_rig_records            a null or destroyed rig (the rig of a destroyed pose is destroyed); null locals with n_parts > 0;
 *                             local_bytes != n_parts * 48; null records_out; record_bytes != n_parts * 96.
 *   pt_rig_clip_records       a null or destroyed rig; no clip attached; a NaN t; null records_out; record_bytes != n_parts * 96.
 *   pt_rig_clip_attach        a null or destroyed rig; n_keys < 1; null times, or null values with n_parts > 0; time_bytes != n_keys * 4;
 *                             value_bytes != n_keys * n_parts * 48; times not finite or not strictly increasing.
 *   pt_rig_pose_geometry      null ctx; a null or destroyed rig; a rig whose pose was created on another context; null locals with n_parts > 0;
 *                             local_bytes != n_parts * 48; ellip_bytes not a multiple of 4.  Then pt_pose_geometry's PT_ERR_SCENE refusals under
 *                             this call's name.
 *   pt_rig_clip_pose_geometry null ctx; a null or destroyed rig; a rig whose pose was created on another context; no clip attached; a NaN t;
 *                             ellip_bytes not a multiple of 4.  Then likewise.
 *
 * OWNERSHIP.  A rig belongs to its pose: pt_pose_destroy and pt_destroy destroy it.  A destroyed rig is refused, not followed, for as long as
 * its address is not reused.  ORDER and threads: as include/pt_pose.h.  pt_debug_rig_time (include/pt_debug.h) times the rig's launches.
 *
 * SEVERAL CLIPS AT ONCE (cross-fades, masked and additive layers, loops): include/pt_rig_mix.h.
 * GOALS IN WORLD SPACE (two-bone chains and aims solved between a call's locals and its levels): include/pt_rig_ik.h.
 *
 * NOT BUILT: sparse per-channel tracks, slerp, cubic keys, joints that write no record.
 */
#ifndef PT_RIG_H
#define PT_RIG_H
#include "pt_pose.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_rig pt_rig;

#define PT_RIG_LOCAL_FLOATS 12      /* t.x t.y t.z pad | q.x q.y q.z q.w | s.x s.y s.z pad */
#define PT_RIG_MAX_DEPTH 256

int pt_rig_create(pt_pose* pose, const int32_t* parent, size_t parent_bytes,
                  const float* inv_bind, size_t bind_bytes,        /* n_parts x 12 floats, 3x4 row-major; NULL: none */
                  pt_rig** out);
int pt_rig_records(pt_rig* rig, const float* locals, size_t local_bytes, float* records_out, size_t record_bytes);
int pt_rig_pose_geometry(pt_ctx* ctx, pt_rig* rig, const float* locals, size_t local_bytes,
                         const float* ellip, size_t ellip_bytes, double* root_cost, int* in_place);
int pt_rig_clip_attach(pt_rig* rig, int n_keys, const float* times, size_t time_bytes, const float* values, size_t value_bytes);
int pt_rig_clip_records(pt_rig* rig, float t, float* records_out, size_t record_bytes);
int pt_rig_clip_pose_geometry(pt_ctx* ctx, pt_rig* rig, float t, const float* ellip, size_t ellip_bytes, double* root_cost, int* in_place);
void pt_rig_destroy(pt_rig* rig);

#ifdef __cplusplus
}
#endif
#endif
