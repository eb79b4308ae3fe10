/* include/pt_pose.h — animate a scene's triangles by per-part matrices, all on the device (libpt_hip.so).
 *
 * No reference counterpart.  include/pt_move.h took the host layout and the record uploads out of an animation step; what remained was host
 * traffic: binding 3 going up, binding 10 coming down, the host copies rewritten.  A caller who animates rigid or affine parts has 12 numbers per
 * part to say.  A pose object lets that caller say them: the posed binding 3, the refit, the patch of the context's records are made on the
 * device, and the context's host copies of bindings 3 and 10 are brought up to date only when something reads them.
 *
 * A POSE OBJECT (pt_pose_create) holds
 *   - the rest pose: the context's binding 3 at creation, 40 floats per triangle, on the device;
 *   - a part id per triangle, tri_part[k] in [-1, n_parts).  Part -1 is static: its triangles are the rest pose's, bit for bit;
 *   - a refit plan of its own (include/pt_refit.h) over the context's bindings 10-13.
 * (include/pt_skin.h makes a pose object under a second rule — up to four records blended per corner — that every call below takes as well.)
 * (include/pt_normals.h attaches vertex ids to a pose object of either kind: the normals are then recomputed from the posed surface after the rule.)
 * (include/pt_rig.h attaches a joint hierarchy to a pose object of any kind: the records are then made on the device from local joint transforms.)
 * (include/pt_rig_mix.h mixes several keyed clips of such a rig, layered and masked per joint, into those transforms on the device.)
 * (include/pt_morph.h attaches morph targets to a pose object of either kind: the rule then starts from the morphed rest pose.  NOT BUILT for
 *  any of the three: posed ellipsoids; JNI natives; rebuilding degraded trees.)
 *
 * THE RULE.  A pose is n_parts records of 24 floats:
 *     floats  0-11   M, 3 x 4, row-major: for points
 *     floats 12-20   N, 3 x 3, row-major: for normals
 *     floats 21-23   padding, ignored
 * The posed triangle k of part p >= 0 replaces 18 floats of the rest triangle.  With (x, y, z) a vertex at floats 0-2, 4-6 or 8-10:
 *     out_i = ((m_i0*x + m_i1*y) + m_i2*z) + m_i3          i = 0, 1, 2
 * and with (x, y, z) a normal at floats 12-14, 16-18 or 20-22:
 *     out_i = ((n_i0*x + n_i1*y) + n_i2*z)
 * in binary32, every product rounded before every sum, in that written order: no fused multiply-add.  Floats 3, 7, 11, 15, 19, 23 and 24-39 are
 * the rest pose's.  Nothing is normalised; N is the caller's to supply (the Python layer offers the inverse transpose of M's linear part,
 * computed in binary64 and then rounded).  Poses are absolute against the rest pose, never cumulative: nothing drifts.
 * An identity M is NOT a no-op: -0.0 becomes +0.0 (the sum with a +0.0 product), and an infinite coordinate becomes NaN (inf * 0).  Part -1 is
 * the way to leave triangles alone.
 *
 * pt_pose_geometry — CONTRACT.  After success the context is in the state that
 *     pt_move_geometry(ctx, plan, P, tri_bytes, ellip, ellip_bytes, root_cost, in_place)
 * would leave it in, where P is the rule applied to the rest pose and plan a refit plan of the context's scene: every device record array byte
 * for byte, every mode, the image-history bookkeeping (bindings 3, 10 and, when given, 7 count as accepted uploads), the host copies as any
 * later reader sees them, root_cost, and the same slow paths reported through in_place.  On the in-place path no triangle data crosses the bus:
 * the call uploads xforms and, when given, the ellipsoids, and downloads two flags, the root costs, the context's root and group records (a few
 * kilobytes, whose references and padding stay) and the rows of binding 10 that those records need (per object its root's and the root's two
 * children's, gathered on the device).
 *
 * HOST COPIES BEHIND THE DEVICE.  After an in-place pose the context's host copies of bindings 3 and 10 are behind: the posed binding 3 and the
 * refit binding 10 lie in the pose's plan.  Every reader of those copies settles first — downloads both and clears the flag: the scene build
 * (after an option or upload that dirties the scene), pt_move_geometry, pt_set_buffer of a scene binding (3, 7, 10-13; it settles before it
 * stores), pt_pose_create, and pt_pose_destroy of the pose the context is behind on.  A second pt_pose_geometry does not settle: it supersedes
 * the first.
 * include/pt_motion.h does not settle either: while the copies are behind, pt_motion_mark and pt_reproject_frame_moved / _bilinear make their
 * triangle records on the device, from the posed binding 3 where it lies — the first 48 bytes of each triangle, the moved flag 0 iff all nine
 * floats compare equal to the mark's record, a triangle beyond the mark's count moved: the host code's records exactly.  Ellipsoids stay on the
 * host path.  A mark taken on the device whose reprojection finds the host copies current again fetches its host positions from those records.
 * An accepted pt_set_buffer of binding 3 or 10-13, or a pt_move_geometry, makes the context's poses stale: their rest pose or trees are no longer
 * the context's, and the next pt_pose_geometry returns PT_ERR_SCENE.
 *
 * SLOW PATHS (in_place = 0; never refused): a multi-stream / multi-GPU context (pt_pose_create works from the first stream's copies;
 * pt_pose_geometry poses on the first device, downloads P and performs pt_move_geometry's sequence), and every slow path of pt_move_geometry.
 *
 * REFUSALS leave the context's records, its image and what a later settle would deliver as they were.  In this order:
 *   pt_pose_create    PT_ERR_ARG: null ctx, tri_part or out; part_bytes != n_tris * 4; n_parts outside [0, 65536]; a part id outside [-1, n_parts).
 *                     Then whatever the scene build returns for a dirty scene that does not build, and pt_refit_create's refusals.
 *   pt_pose_geometry  PT_ERR_ARG: null ctx; null or destroyed pose; a pose of another context; null xforms with n_parts > 0;
 *                     xform_bytes != n_parts * 96; ellip_bytes not a multiple of 4.
 *                     PT_ERR_SCENE: the scene was uploaded since pt_pose_create; binding 7's refusals of pt_move_geometry with the scene
 *                     build's texts; a NaN among the posed vertex floats of a referenced triangle ("pt_pose_geometry: NaN coordinate in a
 *                     referenced triangle": pt_move_geometry's refusal under this call's name).  (The material refusal cannot occur: floats
 *                     36 are the rest pose's, which the scene build accepted.)
 *   pt_pose_triangles PT_ERR_ARG: null or destroyed pose; null xforms with n_parts > 0; xform_bytes != n_parts * 96; null tris_out;
 *                     tri_bytes != n_tris * 160.
 * The NaN flag is read before the first store into a record of the context, but by then the pose's working copies (the plan's binding 3 and
 * binding 10) hold the refused pose.  The pose keeps the matrices of the last accepted pose (none: the rest pose) and, when the context is behind
 * on it, RUNS POSE + REFIT AGAIN WITH THEM before it returns the refusal, so that a later settle delivers the last accepted pose.  (A second pair
 * of buffers would save that rerun at 160 bytes per triangle; refusals are rare, memory is not.)
 *
 * pt_pose_triangles is the rule alone: P downloaded into tris_out.  It changes nothing of the context or of what a settle delivers.
 *
 * OWNERSHIP.  A pose belongs to the context it was created on; pt_destroy destroys it.  A destroyed pose is refused for as long as its address is
 * not reused.  ORDER: as pt_move_geometry — the call completes a running frame stream first and is synchronous.  Not thread-safe per context.
 */
#ifndef PT_POSE_H
#define PT_POSE_H
#include "pt_move.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_pose pt_pose;

#define PT_POSE_MAX_PARTS 65536
#define PT_POSE_RECORD_FLOATS 24

int pt_pose_create(pt_ctx* ctx, const int32_t* tri_part, size_t part_bytes, int n_parts, pt_pose** out);
int pt_pose_geometry(pt_ctx* ctx, pt_pose* pose,
                     const float* xforms, size_t xform_bytes,   /* n_parts records of 24 floats; may be NULL when n_parts == 0 */
                     const float* ellip, size_t ellip_bytes,    /* new binding 7, or NULL: unchanged */
                     double* root_cost,                         /* may be NULL: one double per root */
                     int* in_place);                            /* may be NULL; 1: records patched, 0: rebuilt */
int pt_pose_triangles(pt_pose* pose, const float* xforms, size_t xform_bytes, float* tris_out, size_t tri_bytes);
void pt_pose_destroy(pt_pose* pose);

#ifdef __cplusplus
}
#endif
#endif
