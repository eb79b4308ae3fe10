/* include/pt_skin.h — blend-weight skinning of a scene's triangles, all on the device (libpt_hip.so).
 *
 * No reference counterpart.  include/pt_pose.h moves a triangle by ONE record, so it moves rigid or affine parts; what bends (a limb, a cloth
 * strip, a tube) tears along the part boundary.  A SKINNED POSE is a pt_pose whose rule blends up to four records per CORNER of a triangle.  It
 * is created by pt_skin_create and then used with pt_pose_geometry, pt_pose_triangles and pt_pose_destroy exactly as a pose of pt_pose_create: the
 * same n_parts records of 24 floats (M at 0-11, N at 12-20, padding ignored), the same contract (the state pt_move_geometry of the posed triangles
 * would leave), the same refusals, staleness, slow paths, behind / settle behaviour and ownership.  Only the rule differs.
 *
 * THE TABLES.  12 words per triangle each: corner c (0..2), slot s (0..3) at 12*k + 4*c + s.
 *   corner_bone    the slots of a corner are packed: slots 0..n-1 hold bone ids in [0, n_parts), the remaining slots hold -1
 *   corner_weight  the weight of each used slot; the weights of the slots that hold -1 are ignored (they may be NaN)
 * A corner with n = 0 is STATIC: its vertex float4 and its normal float4 are the rest pose's, bit for bit, and no kernel ever writes them.
 * Corner c owns the vertex at floats 4c..4c+2 and the normal at floats 12+4c..12+4c+2 of its triangle.  Floats 3, 7, 11, 15, 19, 23 and 24-39
 * are always the rest pose's.
 *
 * THE RULE.  For a corner with n >= 1 form the blended record B float by float, j = 0..11 for the vertex and j = 12..20 for the normal, with
 * b_s and w_s the corner's bone ids and weights and X[b] the record of bone b:
 *     B_j = w_0 * X[b_0][j]
 *     B_j = B_j + (w_s * X[b_s][j])          s = 1 .. n-1, in that order
 * in binary32, every product rounded before every sum, nothing fused.  Then include/pt_pose.h's rule with B in place of the part's record: the
 * corner's vertex under B's M, its normal under B's N.  Nothing is normalised: weights need not sum to 1 and may be negative.  Poses are absolute
 * against the rest pose.  Two consequences:
 *   1. w * m with w = 1.0f is exact, so a skin whose every corner of triangle k has the single slot (tri_part[k], 1.0) — no slot where tri_part[k]
 *      is -1 — gives pt_pose_triangles' output of the pose made from tri_part, bit for bit.
 *   2. binding 3 stores a vertex once per triangle that uses it: two corners with the same rest floats and the same 4 + 4 skin words get the same
 *      bits, so a shared vertex does not crack.
 *
 * REFUSALS of pt_skin_create, each check over the whole table before the next, all PT_ERR_ARG under the call's name, in this order:
 *   1. null ctx, corner_bone, corner_weight or out
 *   2. bone_bytes != n_tris * 48
 *   3. weight_bytes != n_tris * 48
 *   4. n_parts outside [0, 65536]
 *   5. a bone id outside [-1, n_parts)
 *   6. a bone id after an empty slot
 *   7. a weight of a used slot that is not finite
 * Then whatever pt_pose_create returns after its argument checks: the scene build's refusals for a dirty scene that does not build, and
 * pt_refit_create's.  pt_debug_pose_time (include/pt_debug.h) refuses a skinned pose with PT_ERR_ARG: it launches the kernels of the one-record
 * rule on a part table the skin does not have; pt_debug_skin_time times the skin's.
 *
 * (Morph targets — per-corner offsets under one weight per target, applied to the rest pose ahead of this rule — are include/pt_morph.h's.)
 * (Normals recomputed from the skinned surface, instead of the blended N this rule applies, are include/pt_normals.h's.)
 * (Dual-quaternion blending — the same tables under a rule that keeps the volume of what twists, where this one's blended matrix shrinks it —
 * is include/pt_skin_dq.h's, pt_skin_dq_create.)
 * NOT BUILT: more than four slots; 16-bit packed tables (48 bytes per triangle instead of 96); posed ellipsoids; JNI
 * natives; rebuilding degraded trees.
 */
#ifndef PT_SKIN_H
#define PT_SKIN_H
#include "pt_pose.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PT_SKIN_SLOTS 4

int pt_skin_create(pt_ctx* ctx,
                   const int32_t* corner_bone, size_t bone_bytes,      /* 12 per triangle: corner c (0..2), slot s (0..3) at 12*k + 4*c + s */
                   const float* corner_weight, size_t weight_bytes,    /* same indexing */
                   int n_parts, pt_pose** out);

#ifdef __cplusplus
}
#endif
#endif
