/* include/pt_through.h — "seen-through" feature records: the records of include/pt_denoise.h followed through mirrors and glass, and the prefill
 * and guided filter of include/pt_fill.h run on them, on top of include/pt_api.h (libpt_hip.so).
 *
 * No reference counterpart.  The first-hit records give every pixel of a polished sphere the sphere's own smooth normal and depth, so the fill,
 * the pooled variance and the filter blend the different things seen IN it.  chooseRay's reflection lobe is always the exact mirror direction
 * (the rough vector is mixed in with weight 0, frag.glsl:775) and its transmission lobe an exact refract (:783), so every pixel has a
 * deterministic chain of delta lobes; the record below is the one of the surface at the chain's end.  Every call of the other headers stays
 * exactly as it is; these are opt-in.  Nothing here changes FRAME, T or the render path.  Steering, selection and reprojection stay on the
 * first-hit records (reprojection needs the real geometry).
 *
 * Chain of a pixel.  Under the exact numeric contract whatever pt_set_option 16 says.  State: the lens-centre ray (O, D0) of
 * include/pt_denoise.h, D = D0; trace()'s initial index stack {1.0029} (:816; every other slot holds 0.0); tint = (1, 1, 1), L = 0, k = 0.  Repeat:
 *   1. rayScene(O, D).  A miss ends the chain: the record is the one written last, or the first-hit miss record when there is none.
 *   2. Decode the hit as trace() does (:823-840): mapMtl, the map_norm texel, ND = dot(N, D), Nf = N flipped towards the ray, n1, n2 and the
 *      push (ND < 0) or pop of the index stack, with its stale-slot and full-stack behaviour; L += the segment's t.
 *   3. Write the surface's record S (the layout of include/pt_denoise.h):
 *        S0 = (L, N.x, N.y, N.z)                N before the flip
 *        S1 = (tint * Kd per component, hit)    Kd after mapMtl; the products in chain order, ((1 * Kd_0) * Kd_1) * ...; hit code of THIS surface
 *        S2 = (D0.x, D0.y, D0.z, surface word)  the material index when k == 0 or PT_THROUGH_KEY is off,
 *                                               else (k << 24) | (first-hit material << 12) | material, as int32 bits
 *        S3 = (u, v, k as int32 bits, 0)
 *   4. Stop if k == max_depth.
 *   5. chooseRay's weights (:745-765), no random number drawn: r = 1 - Pr, c = Pc, t = Tr > 0 ? Tr : (Tf.r > 0 ? (Tf.r + Tf.g + Tf.b) / 3 : 0);
 *      if illum is 5 or 7 or t > 0: f = fresnelReflectAmount(n1, n2, Nf, D), r += f * Pr, t *= 1 - f (else f = 0);
 *      d = (1 - Pm) * (1 - t) * (1 - f); total = d + r + c + t; r' = r / total, t' = t / total.
 *   6. Follow reflection if (lobes & PT_THROUGH_REFLECT) and r' >= min_weight and r' >= t'; else transmission if (lobes & PT_THROUGH_TRANSMIT)
 *      and t' >= min_weight; else stop.  A NaN compares false and stops.
 *   7. The direction: reflect(D, Nf), or refract(D, Nf, n1 / n2).  Stop if a component is not finite or the vector is zero (total internal
 *      reflection).
 *   8. tint *= Kd, O = hit.loc, D = the direction, k += 1.
 * reflect(D, Nf) is trace()'s reflection direction wherever the discarded rough vector is finite.  Tint follows trace(): it multiplies by Kd
 * for both lobes; absorption is ignored.  With RAYTRACING == 0 (Parameters[9] != 1) no step is taken.  Reverting to the last record on a miss
 * means that a mirror pixel that sees the sky keeps the mirror's own record, and is never blended with one that sees the floor.
 * max_depth 0 or lobes 0 gives pt_read_features' records bit for bit.
 */
#ifndef PT_THROUGH_H
#define PT_THROUGH_H
#include "pt_api.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { PT_THROUGH_REFLECT = 1, PT_THROUGH_TRANSMIT = 2 };   /* lobes */
enum { PT_THROUGH_KEY = 1 };                                 /* flags */
typedef struct pt_through_rule { int max_depth; float min_weight; int lobes; int flags; } pt_through_rule;
#define PT_THROUGH_RAY_FLOATS 8

/* Every call below:  PT_ERR_ARG: a null rule, max_depth outside 0 .. 8, min_weight NaN or outside (0, 1], lobes outside 0 .. 3, unknown flag
 * bits.  PT_ERR_UNSUPPORTED: PT_THROUGH_KEY in a scene with more than 4096 materials. */

/* Fills out[W*H*16] with the records S above, FRAME's pixel order.  They are kept on the device beside the first-hit records and recomputed
 * when pt_set_buffer or pt_set_texture was called since the last computation or the rule differs from the last call's, otherwise reused.
 * Synchronous; works on every context, and later renders are bit-identical to renders without this call, as with pt_read_features.
 * Errors as pt_read_features. */
int pt_read_features_through(pt_ctx* ctx, const pt_through_rule* rule, float* out);
/* The parity probe: out[W*H*8], per pixel (O.x, O.y, O.z, t, D.x, D.y, D.z, k as int32 bits) of the segment that found the recorded surface —
 * rayScene(O, D) hits it at distance t.  A pixel whose first ray misses has the lens-centre ray, t = -1 and k = 0.  Cached with the records. */
int pt_read_through_rays(pt_ctx* ctx, const pt_through_rule* rule, float* out);
/* pt_fill_frame, pt_denoise_guided_filled and pt_read_display_denoised_guided_filled of include/pt_fill.h word for word, with S in place of
 * the first-hit records: albedo_floor 0 gives the plain rule, an image without holes the plain or demodulated guided filter.  Errors are
 * theirs, and the rule's above. */
int pt_fill_frame_through(pt_ctx* ctx, const pt_through_rule* rule, float sigma_normal, float sigma_depth, float sigma_albedo, float albedo_floor,
                          float* rgba_out, int64_t* n_filled);
int pt_denoise_guided_through(pt_ctx* ctx, const pt_through_rule* rule, int iterations, float sigma_lum, float sigma_normal, float sigma_depth,
                              float sigma_albedo, int min_frames, float albedo_floor, float* rgba_out);
int pt_read_display_denoised_guided_through(pt_ctx* ctx, const pt_through_rule* rule, int iterations, float sigma_lum, float sigma_normal,
                                            float sigma_depth, float sigma_albedo, int min_frames, float albedo_floor, int java_bytes, uint8_t* rgb_out);

#ifdef __cplusplus
}
#endif
#endif
