/* include/pt_normals.h — smooth normals recomputed from the posed surface, all on the device (libpt_hip.so).
 *
 * No reference counterpart.  include/pt_pose.h, include/pt_skin.h and include/pt_morph.h carry normals by approximation: the pose rule multiplies a
 * normal by the caller's N, the skin blends N per corner, a morph adds a caller-supplied dn scaled by its weight.  None of them looks at the
 * surface the step produced, and a caller whose deformation is not small, or whose data hold positions only (a simulation cache, a cloth strip, a
 * height field driven by a few modes, a strongly bent skin), has no correct normal to hand in.  NORMALS attached to a pose object — one of
 * pt_pose_create or of pt_skin_create, with or without a morph — recompute the vertex normals from the posed triangles as the last stage of the
 * pose's rule: morph, skin, NORMALS, refit, patch.  Everything else is the pose's: pt_pose_geometry still ends in the state pt_move_geometry of the
 * posed triangles P would leave, and P now includes the recomputed normals; refusals, staleness, slow paths, behind / settle behaviour are unchanged.
 * Attached once and destroyed with the pose; there is no detach: mode 0 takes its place.
 *
 * THE TABLE.  corner_vertex holds three ids per triangle, corner c of triangle k at 3*k + c, each in [-1, n_vertices).  Corners with the same
 * id >= 0 are ONE vertex of the surface and receive the same recomputed normal.  A corner with -1 keeps the normal the pose's rule wrote.  An id
 * that no corner names is allowed.
 *
 * THE RULE, in binary32, every product rounded before every sum, in the written order, nothing fused.  It runs after the pose's rule (or the
 * skin's, morphed or not) has written the posed triangles.
 *   1. the face vector of triangle k, from its three posed vertices v0 v1 v2 (floats 0-2, 4-6, 8-10; static corners included):
 *          e1 = v1 - v0, e2 = v2 - v0,  F = (e1.y*e2.z - e1.z*e2.y,  e1.z*e2.x - e1.x*e2.z,  e1.x*e2.y - e1.y*e2.x)
 *      with PT_NORMALS_FLIP each component negated (exact);
 *   2. the sum of vertex g over the corners that name g in ascending corner index q: S = F[q_0 / 3], then S_j = S_j + F[q_i / 3]_j in that order.
 *      The weights are the areas (twice over); no angle weights;
 *   3. L = sqrt((S.x*S.x + S.y*S.y) + S.z*S.z), correctly rounded; if L is finite and > 0, N_j = S_j / L with a correctly rounded divide;
 *   4. otherwise every corner of g keeps what the pose's rule wrote: a degenerate fan, an underflowed or overflowed square, an infinity or a NaN
 *      among the vertices;
 *   5. N goes to floats 12+4c .. 12+4c+2 of each corner of g.  Floats 15, 19, 23 and everything else keep their values.
 * Consequences:
 *   - a recomputed normal is always finite;
 *   - corners of one vertex get the same bits: no shading seam where binding 3 stores a vertex once per triangle;
 *   - with mode 0 the output is, bit for bit, that of the same pose without the attach;
 *   - with xforms == NULL (the rest pose) nothing is recomputed: the rest pose stays the rest pose;
 *   - on a planar fan with consistent winding whose triangles have the same, exactly computed face vector every corner gets the same bits
 *     (a rim vertex sums 2 F, the centre n F).  On any planar fan the corners agree as far as the rounding of the face vectors and of the sums
 *     lets them; in a plane normal to an axis every corner gets that axis, where an exact zero may carry either sign.
 * The shader interpolates only where all three components of corner 0's normal are non-zero (frag.glsl:501-504), and it uses vn1
 * and vn2 only.  A recomputed normal with an exact zero component at corner 0 sends that triangle to its face normal, as any such normal always
 * did: that is the oracle's business and is not changed here.
 *
 * WHICH CORNERS.  An id >= 0 is allowed only on a corner that the pose's rule moves: tri_part[k] >= 0, or under a skin a bone in slot 0
 * (pt_morph_attach's check 11).  Static corners stay written once, at creation, and by no kernel.  At a boundary between moved and static
 * triangles a moved vertex therefore sums the triangles on its moved side only (the face vectors of those triangles do read their static
 * corners' positions).
 *
 * pt_normals_attach — the mode is 1 afterwards.  PT_ERR_ARG under the call's name, each check over the whole table before the next, in this order:
 *    1. a null or destroyed pose, or a null corner_vertex
 *    2. the pose has normals attached already
 *    3. a bit of flags other than PT_NORMALS_FLIP
 *    4. n_vertices outside [0, 3 * n_tris]
 *    5. vertex_bytes != n_tris * 12
 *    6. an id outside [-1, n_vertices)
 *    7. the same id >= 0 at two corners of one triangle
 *    8. an id >= 0 at a corner the pose's rule leaves static
 * Then PT_ERR_SCENE when the pose is stale (the scene was uploaded since pt_pose_create).
 *
 * pt_normals_mode — 0: the pose rule's normals, 1: recomputed.  A host-side store like pt_morph_weights: it changes nothing of the context or of
 * what a settle would deliver, does not flush a running frame stream, and applies to the next pt_pose_geometry / pt_pose_triangles.  PT_ERR_ARG: a
 * null or destroyed pose; a pose without normals; on outside {0, 1}.
 *
 * Nothing else is refused later.  THE LAST ACCEPTED POSE is the triple (records, weights, mode): a refusal while the context is behind on the pose
 * runs pose and refit again with all three, so that a later settle delivers them; a pose accepted before the attach counts as accepted with mode 0.
 *
 * (A pose of pt_skin_dq_create, include/pt_skin_dq.h, takes normals as a pose of pt_skin_create does: they are recomputed from what its rule wrote.)
 * NOT BUILT: angle weights; a crease angle (scenes.weld_corners keeps hard edges by the rest normals instead); a detach; a scaled sum that
 * survives the overflow of the square; JNI natives.
 */
#ifndef PT_NORMALS_H
#define PT_NORMALS_H
#include "pt_pose.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PT_NORMALS_FLIP 1u

int pt_normals_attach(pt_pose* pose,
                      const int32_t* corner_vertex, size_t vertex_bytes,  /* 3 per triangle: corner c of triangle k at 3*k + c */
                      int64_t n_vertices, uint32_t flags);
int pt_normals_mode(pt_pose* pose, int on);   /* 0: the pose rule's normals, 1: recomputed; after the attach: 1 */

#ifdef __cplusplus
}
#endif
#endif
