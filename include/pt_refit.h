/* include/pt_refit.h — refit a scene's BVHs to moved triangles on the GPU (libpt_hip.so).
 *
 * No reference counterpart: the reference builds every tree once.  include/pt_motion.h lets the caller move primitives between the mark and
 * pt_reproject_frame_moved and expects bindings 3, 7, 10, 11, 12 and 13 uploaded in between.  Under that header's rule (triangle k stays the
 * same piece of surface; only its position changes) the old topology, bindings 11, 12 and 13, is still a valid tree over the moved triangles,
 * and only the boxes of binding 10 are stale.  The three calls here recompute them: a plan holds the topology on the device, every run takes
 * a new binding 3 and returns the new binding 10.  No pt_ctx is involved (as pt_build_bvh has none): the caller uploads the result with
 * pt_set_buffer like any other buffer, and a refit tree is an ordinary input to every render path.
 *
 * Buffers.  Binding 10: 8 floats per node, [min x y z, max x y z, leafStart, leafEnd].  Binding 11: 3 ints per node, [id, left, right];
 * a leaf has left == right == -1.  Binding 12: triangle ids, the leaves' ranges index it.  Binding 13: [count, root id x count].  Binding 3:
 * 40 floats per triangle, of which floats 0-2, 4-6 and 8-10 are the three vertices.  n_nodes is the row count of binding 11; binding 10 must
 * hold at least as many rows.
 *
 * Boxes.  Binary32 values are compared in the order in which -0.0 < +0.0, as Java's Math.min / Math.max have it (the reference's
 * GrowToInclude); nothing is rounded.
 *   - A leaf's box is the component-wise min and max over the nine vertex floats of the triangles leaf_tris[leafStart .. leafEnd).
 *   - An inner node's box is the union of its two children's boxes, in the same order.
 *   - An empty leaf (leafStart == leafEnd) keeps the box it had at pt_refit_create and takes part in its parent's union with it.
 *   - Rows of nodes that no root reaches, and rows of binding 10 beyond n_nodes, are copied unchanged from pt_refit_create's bvh_data.
 *   - Floats 6 and 7 of every row are copied unchanged.
 * min and max do not round, and the reference packs (float) of double boxes that are tight around the vertices it packs as (float), and
 * rounding is monotone.  So the result does not depend on the order of evaluation, and a refit with the scene's own binding 3 gives back its
 * own binding 10 bit for bit.
 *
 * Cost.  For the caller to decide when a rebuild pays; compared with the same number from a run on the rest pose.  Binary64, in the written
 * order, no fused multiply-add; min and max are the node's new box:
 *   s = (double)max - (double)min per axis;  A = (s.x*s.y + s.x*s.z) + s.y*s.z
 *   S(leaf) = A * (double)(leafEnd - leafStart);  S(inner) = A + (S(left) + S(right));  root_cost[r] = S(root r), r in binding 13's order.
 * Each node's value is a fixed expression of its children's stored values, so it is deterministic as well.
 *
 * Limits: n_nodes <= 2^27, n_tris <= 2^30, leaf_tris no longer than 2^30 entries.
 */
#ifndef PT_REFIT_H
#define PT_REFIT_H
#include "pt_api.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_refit_plan pt_refit_plan;

/* Validates the four buffers, plans the refit (parents, heights, the nodes grouped by height: csrc/hip/pt_refit_plan.hpp) and keeps the plan
 * and a copy of bvh_data on `device`.  The buffers are not referenced after the call.
 * PT_ERR_ARG: a null pointer; data_bytes not a multiple of 32, tree_bytes of 12, leaf_bytes or roots_bytes of 4; roots_bytes < 4;
 * n_tris < 0; a count beyond the limits above.
 * PT_ERR_SCENE: binding 10 shorter than binding 11's rows; a tree row whose id is not its index; one child without the other; a child
 * outside (id, n_nodes) (the reference numbers in pre-order, so this refuses every cycle); a root count that exceeds binding 13; a root out
 * of range; a node with two parents or reached from two roots; a reachable leaf whose range is not integral or not within
 * 0 <= start <= end <= leaf count; a triangle id of such a range outside [0, n_tris).
 * PT_ERR_NO_DEVICE: no gfx950 device at that index.  PT_ERR_HIP: a runtime call failed.  *out is written on success only. */
int pt_refit_create(int device,
                    const float* bvh_data, size_t data_bytes,     /* binding 10 */
                    const int32_t* bvh_tree, size_t tree_bytes,   /* binding 11 */
                    const int32_t* leaf_tris, size_t leaf_bytes,  /* binding 12 */
                    const int32_t* obj_roots, size_t roots_bytes, /* binding 13 */
                    int64_t n_tris, pt_refit_plan** out);

/* One refit: tris is the new binding 3 (tri_bytes == n_tris * 160), bvh_data_out receives data_bytes of the new binding 10, root_cost (may be
 * NULL) one double per root.  Synchronous; a plan may be run any number of times, each run starts from the triangles alone.  Not
 * thread-safe per plan.
 * PT_ERR_ARG: a null or destroyed plan, null tris or bvh_data_out, tri_bytes != n_tris * 160.
 * PT_ERR_SCENE: a NaN among the nine vertex floats of a triangle that a reachable leaf references (pt_build_bvh refuses the same;
 * infinities are allowed).  On this refusal, as on every other, bvh_data_out and root_cost are not written. */
int pt_refit_run(pt_refit_plan* plan, const float* tris, size_t tri_bytes, float* bvh_data_out, double* root_cost);

/* Frees the plan's device memory.  NULL is ignored.  A destroyed plan is refused by pt_refit_run as long as its address is not reused. */
void pt_refit_destroy(pt_refit_plan* plan);

#ifdef __cplusplus
}
#endif
#endif
