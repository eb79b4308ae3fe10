/* include/pt_move.h — move a scene's triangles in place: refit the BVHs and patch the context's device records (libpt_hip.so).
 *
 * No reference counterpart.  include/pt_refit.h took the rebuild of the trees out of an animation step; what remained was that the uploads of
 * bindings 3 and 10 make the next render lay the whole scene out again on the host and upload every record array.  Under include/pt_motion.h's
 * rule (triangle k stays the same piece of surface, topology unchanged) only a narrow part of those records depends on the coordinates of
 * binding 3 and the boxes of binding 10:
 *   - floats 0-8 of each 48-byte triangle record (v1, e1, e2);
 *   - the 64-byte shading records;
 *   - the box floats of the 64-byte node records and of the hand-written kernel's 80- or 64-byte node records;
 *   - the root boxes, the 64 group boxes of scenes with more than 8 BVHs and their never-cull flag;
 *   - whether every node box is ordered.
 * Everything else — the order of the records, every reference, the triangle-to-object table, the strides, the stack depth, the LDS splits,
 * materials and textures — is a function of bindings 11-13 and 14, the textures and the options.  pt_move_geometry rewrites exactly the former on
 * the device, from the plan's device copies of the new binding 3 and the refit binding 10.
 *
 * CONTRACT.  After a successful call the context is in the state that
 *     pt_refit_run(plan, tris, ...);  pt_set_buffer(ctx, 3, tris);  pt_set_buffer(ctx, 10, <refit result>);  [pt_set_buffer(ctx, 7, ellip);]
 * followed by the scene build of the next render would leave it in: the same host copies of the bindings, every device record array byte for
 * byte, every mode taken from the layout, and the same bookkeeping of what the current image is a picture of — the record caches are dropped,
 * bindings 3, 10 and (when given) 7 count as accepted scene uploads, so the mark of pt_motion_mark stays valid as it does across those uploads.
 * The call therefore stands in place of those uploads between pt_motion_mark and pt_reproject_frame_moved / _bilinear.  The scene is built (not
 * dirty) afterwards.
 *
 * in_place (may be NULL) receives 1 when the records were patched on the device — no host layout, no record array uploaded except the few
 * kilobytes of root, group and ellipsoid records, which the host computes from the downloaded binding 10 — and 0 when the call performed the
 * sequence above literally and built the scene.  The slow path is taken, never refused, when a patch cannot promise equality:
 *   - a multi-stream / multi-GPU context: every replica takes the uploads and builds;
 *   - the built layout had a node box with min > max or a NaN in 80-byte node records and no empty leaf: it was not eligible for the hand-written
 *     intersect kernel, and refit boxes of non-empty leaves are always ordered, so a layout of the new buffers would be;
 *   - ellip is given and changes the ellipsoid count or any ellipsoid's material index (whether an ellipsoid carries a mapped material could
 *     change);
 *   - the context's binding 3 holds another number of triangles than the plan was made for (found while building this; the sequence above is
 *     legal there as long as the leaves' ids fit, but the shading records change their size);
 *   - the patch kernels report a node box that is not ordered where the modes assume ordered boxes (cannot happen with refit boxes; kept as a
 *     check: the call then builds the scene from the host copies).
 *
 * REFUSALS.  The context's scene and records stay as they were:
 *   PT_ERR_ARG    a null ctx, a null or destroyed plan, null tris; tri_bytes != n_tris * 160 (the plan's n_tris); ellip_bytes not a multiple of 4;
 *                 the plan lives on another device than the context.
 *   PT_ERR_SCENE  the plan was not made from this context's scene: a 64-bit digest of bindings 11, 12 and 13, of floats 6-7 of every row of
 *                 binding 10 and of the four lengths, kept by pt_refit_create, differs from the digest of the context's host copies;
 *                 a NaN among the vertex floats of a referenced triangle (pt_refit_run's refusal);
 *                 a referenced triangle whose material index is outside [0, materials) (the scene build's refusal, its text);
 *                 binding 7 shorter than its count says, or an ellipsoid material index out of range (the scene build's texts).
 *   Whatever the scene build returns when the scene was dirty on entry and does not build.
 * Every check that runs on the device (the NaN flag, the material flag) is read before the first store into a record of the context; the refit
 * itself writes the plan's working copy only.  On a multi-stream context the scene build's own refusals (material indices) come from
 * pt_set_buffer's sequence as they would from the sequence above: the uploads have then happened.
 *
 * ORDER.  The call completes a running frame stream first (submitted frames are rendered in the old scene), as an upload followed by a render
 * does, and is synchronous.  The plan's stream and the context's stream are ordered by host synchronisation.  Not thread-safe per plan or
 * per context.  A plan may serve several contexts that hold the same topology; its map of the record order is remade when bfs_nodes
 * (pt_set_option 10) differs from the call before.
 */
#ifndef PT_MOVE_H
#define PT_MOVE_H
#include "pt_refit.h"
#ifdef __cplusplus
extern "C" {
#endif

int pt_move_geometry(pt_ctx* ctx, pt_refit_plan* plan,
                     const float* tris, size_t tri_bytes,       /* new binding 3 */
                     const float* ellip, size_t ellip_bytes,    /* new binding 7, or NULL: unchanged */
                     double* root_cost,                         /* may be NULL: one double per root, as pt_refit_run */
                     int* in_place);                            /* may be NULL; 1: records patched, 0: rebuilt */

#ifdef __cplusplus
}
#endif
#endif
