/* include/pt_morph.h — morph targets (blend shapes) ahead of the pose rule, all on the device (libpt_hip.so).
 *
 * No reference counterpart.  include/pt_pose.h moves rigid or affine parts and include/pt_skin.h what bends; neither says what a face, a muscle
 * bulge or a simulation cache expressed as a few modes says: per-vertex offsets scaled by one weight per step.  A MORPH is a table of such targets
 * attached to a pose object — one of pt_pose_create or of pt_skin_create — whose rule then starts from the MORPHED rest pose instead of the rest
 * pose.  Everything after that is the pose's: the same records, pt_pose_geometry's contract (the state pt_move_geometry of the posed triangles
 * would leave), refusals, staleness, slow paths, behind / settle behaviour.  A morph is attached once and destroyed with its pose; there is no
 * detach: all weights zero is the unmorphed pose, bit for bit.
 *
 * THE TABLE.  n_targets targets; target t owns the entries target_start[t] .. target_start[t + 1] - 1 of the two entry arrays, in any order:
 *   entry_corner   q = 3*k + c: corner c (0..2) of triangle k.  A target names a corner at most once
 *   entry_delta    six floats per entry: dx dy dz for the corner's vertex, dnx dny dnz for its normal
 * Corner q owns the vertex at floats 4c..4c+2 and the normal at floats 12+4c..12+4c+2 of triangle k.
 *
 * THE RULE.  The entries of a corner are those of all targets that name it, in ascending target order.  Start from the rest pose's six floats;
 * for each entry in that order, with w = weights[target]:
 *     w == 0.0f (so +0 or -0): the entry is skipped
 *     otherwise   v_j = v_j + (w * d_j)    j = 0, 1, 2        n_j = n_j + (w * dn_j)    j = 0, 1, 2
 * in binary32, every product rounded before every sum, nothing fused.  Floats 3 and 15 of the corner's float4s are carried through, nothing is
 * normalised, weights may be negative or exceed 1.  The result takes the place of the rest pose's floats in pt_pose.h's or pt_skin.h's rule.
 * Morphs are absolute against the rest pose.  Three consequences:
 *   1. with every weight +-0 the output of pt_pose_triangles is that of the same pose without a morph, bit for bit: -0.0 and infinities of the
 *      rest pose included (no sum is made);
 *   2. two corners with the same rest floats, the same entries and the same skin or part words get the same bits: a vertex that binding 3
 *      stores once per triangle does not crack;
 *   3. one entry at weight 1.0f gives the correctly rounded v + d (1.0f * d is exact).
 *
 * WHICH CORNERS.  Only corners that the pose's rule moves may carry entries: those of triangles with tri_part[k] >= 0, or, under a skin, corners
 * whose slot 0 holds a bone.  Static corners are written once, at creation, and no kernel ever writes them; a delta on one is refused.  So a pose
 * with n_parts == 0 takes only a morph without entries: give morph-only triangles a part with an identity record (and mind pt_pose.h's caveat:
 * an identity M is not a no-op on -0.0 and infinities).
 *
 * pt_morph_attach — every weight is 0 afterwards.  PT_ERR_ARG under the call's name, each check over the whole table before the next, in this
 * order, with E = target_start[n_targets]:
 *    1. a null or destroyed pose; null target_start, entry_corner or entry_delta
 *    2. the pose has a morph already
 *    3. n_targets outside [1, 1024]
 *    4. start_bytes != (n_targets + 1) * 8
 *    5. target_start is not 0 = s_0 <= s_1 <= ... <= s_n <= 0x7fffffff
 *    6. corner_bytes != E * 4
 *    7. delta_bytes != E * 24
 *    8. a corner outside [0, 3 * n_tris)
 *    9. the same corner twice in one target
 *   10. a delta that is not finite
 *   11. a corner that the pose's rule leaves static
 * Then PT_ERR_SCENE when the pose is stale (the scene was uploaded since pt_pose_create).
 *
 * pt_morph_weights — the weights that the next pt_pose_geometry and pt_pose_triangles use.  It changes nothing of the context or of what a settle
 * would deliver, and does not flush a running frame stream.  PT_ERR_ARG: a null or destroyed pose; a pose without a morph; null weights;
 * weight_bytes != n_targets * 4; a weight that is not finite.
 *
 * Nothing else is refused later.  An overflow inside the rule gives +-inf and possibly NaN after the pose rule: pt_pose_geometry's NaN refusal
 * catches that, under its own name.  THE LAST ACCEPTED POSE is the pair (records, weights): a refusal while the context is behind on the pose runs
 * pose and refit again with both, so that a later settle delivers them; none accepted yet is the rest pose, unmorphed; a pose accepted before the
 * attach counts as accepted with every weight 0.
 *
 * (A table without normal deltas, or a deformation too large for them: include/pt_normals.h recomputes the normals from the posed surface.)
 * (A pose of pt_skin_dq_create, include/pt_skin_dq.h, takes a morph as a pose of pt_skin_create does: its rule starts from the same morphed rest pose.)
 * NOT BUILT: a detach; more than 1024 targets; 16-bit packed tables; posed ellipsoids; JNI natives; rebuilding degraded trees.
 */
#ifndef PT_MORPH_H
#define PT_MORPH_H
#include "pt_pose.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PT_MORPH_MAX_TARGETS 1024

int pt_morph_attach(pt_pose* pose, int n_targets,
                    const int64_t* target_start, size_t start_bytes,   /* n_targets + 1 offsets into the entry arrays; [0] = 0 */
                    const int32_t* entry_corner, size_t corner_bytes,  /* per entry: 3*k + c, corner c of triangle k */
                    const float* entry_delta, size_t delta_bytes);     /* per entry 6 floats: dx dy dz (vertex), dnx dny dnz (normal) */
int pt_morph_weights(pt_pose* pose, const float* weights, size_t weight_bytes);   /* n_targets floats */

#ifdef __cplusplus
}
#endif
#endif
