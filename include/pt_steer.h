/* include/pt_steer.h — adaptive sampling steered by the variance-guided filter, on top of include/pt_api.h (libpt_hip.so), include/pt_adaptive.h
 * (T, the own-moment rule), include/pt_denoise.h (feature records, pixel classes) and include/pt_guided.h (the guided filter and its variance).
 *
 * No reference counterpart.  pt_render_adaptive stops a pixel by its own moments alone, so a pixel whose first frames happen to agree (four
 * zeros where a rare light path lands) has variance 0 and never resumes.  The rule below asks the guided filter instead: a pixel is rendered
 * while the variance of its FILTERED mean is above the tolerance, and the filter pools noise over the pixel's surface.  With pt_reproject_frame
 * (include/pt_reproject.h) this closes the loop of spatiotemporal variance-guided filtering: move, reproject, render the uncertain pixels,
 * filter.  Disoccluded pixels (n = 0) are active by step 3.
 *
 * Rule, per pixel p of the current image, float32 without contraction, in this order (l(c) = (0.2126*c.r + 0.7152*c.g) + 0.0722*c.b,
 * T_p = (sY, sYY, n, 0), read as zeros when T was never allocated):
 *   1. p under the current MOUSE_POS overlay: inactive.
 *   2. max_frames > 0 and n >= max_frames: inactive.
 *   3. n < min_frames: active.
 *   4. p INVALID as include/pt_denoise.h defines it (FRAME.a <= 0, a non-finite mean, a non-finite t, N or Kd): include/pt_adaptive.h's
 *      own-moment rule on T_p, active iff err2 > tol*tol with mean = sY / n, var = (sYY - sY*mean) / (n - 1), err2 = var / n,
 *      tol = fmaxf(rel_err * fabsf(mean), abs_err).  (The NaN pixels of geometry without vertex normals stay inactive, as there.)
 *   5. otherwise: (c_K, v_K) = the mean and the carried variance of p after K = iterations passes of include/pt_guided.h's filter with the
 *      rule's sigmas and min_frames (K = 0: c_0 = the mean, v_0 = s2 / A); tol = fmaxf(rel_err * fabsf(l(c_K)), abs_err); active iff
 *      v_K == +inf or v_K > tol*tol.  A NaN v_K is inactive.
 * Step 5 inherits the filter's contract: not bit-exact (__expf, sqrtf, the device's summation order) but within the per-pixel bounds on c_K and
 * v_K that tests/_guided_ref64.py derives (wide on nearly converged pixels, see include/pt_guided.h), so a pixel whose v_K lies within them of
 * tol*tol may fall on either side.  Steps 1-4 are exact.
 * The rule assumes every frame of the image went into T: pt_render_mask and pt_render_adaptive_guided guarantee it; frames of pt_render /
 * pt_render_batch / pt_render_batch_async do only while moment recording is on (pt_record_moments, include/pt_guided.h).
 */
#ifndef PT_STEER_H
#define PT_STEER_H
#include "pt_api.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The rule's ten parameters. */
typedef struct pt_guided_rule {
    int iterations;                                            /* K, 0 .. 8, as pt_denoise_guided */
    float sigma_lum, sigma_normal, sigma_depth, sigma_albedo;  /* > 0, not NaN; +inf switches the term off */
    int min_frames;                                            /* >= 2: step 3, and own against pooled s2 in the filter */
    float rel_err, abs_err;                                    /* >= 0, not NaN */
    int max_frames;                                            /* >= 0, 0 = no cap */
} pt_guided_rule;

/* Renders frames first_frame .. first_frame+n_frames-1 (seeds[i] = u_seed of frame first_frame+i) for the pixels with mask[y*W + x] != 0
 * (W*H bytes, FRAME's pixel order: row 0 is the bottom row, as pt_read_frame) and for no other pixel; pixels under the current mouse overlay
 * are skipped whatever the mask says.  FRAME and T are updated exactly as pt_render_adaptive updates them (T allocated zeroed on first use),
 * and every pixel-frame is the reference's own job.  Works on every context: each stream takes its own pixels from the full mask.
 * Synchronous, like pt_render_adaptive.  *n_active (may be NULL) = the number of pixels rendered, summed over the context's streams.
 * PT_ERR_ARG: null context, seeds or mask, n_frames < 1.  PT_ERR_UNSUPPORTED: Parameters.DEBUG != 0. */
int pt_render_mask(pt_ctx* ctx, int first_frame, int n_frames, const int32_t* seeds, const uint8_t* mask, int64_t* n_active);
/* The rule above over the current image into mask_out[W*H] (1 = active, 0 = not; FRAME's pixel order) and *n_active (may be NULL).  FRAME
 * and T are not modified.  Computes the feature records first if they are stale (see pt_read_features).  Synchronous.
 * PT_ERR_ARG: null context, rule or mask_out, a field of the rule outside its range.  PT_ERR_UNSUPPORTED: a context that holds only part of
 * the image (pt_create with shard_count > 1, a pt_create_multi_part group). */
int pt_select_guided(pt_ctx* ctx, const pt_guided_rule* rule, uint8_t* mask_out, int64_t* n_active);
/* pt_select_guided, then pt_render_mask on its mask: FRAME, T and *n_active (may be NULL) are bit for bit those of the two calls made one
 * after the other.  On a one-stream context the mask never leaves the device.
 * PT_ERR_ARG: null context, seeds or rule, n_frames < 1, a field of the rule outside its range.  PT_ERR_UNSUPPORTED: Parameters.DEBUG != 0,
 * a context that holds only part of the image. */
int pt_render_adaptive_guided(pt_ctx* ctx, int first_frame, int n_frames, const int32_t* seeds, const pt_guided_rule* rule, int64_t* n_active);

#ifdef __cplusplus
}
#endif
#endif
