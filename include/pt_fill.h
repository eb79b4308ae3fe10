/* include/pt_fill.h — interleaved rendering: a lattice of pixels rendered, the others reconstructed before the guided filter, on top of
 * include/pt_api.h (libpt_hip.so), include/pt_denoise.h (feature records, pixel classes), include/pt_guided.h (the filter), include/pt_steer.h
 * (pt_render_mask) and include/pt_demod.h (the illumination).
 *
 * No reference counterpart.  pt_render_mask renders any subset of the pixels, every pixel-frame still the reference's own job, but the filters
 * pass a pixel with FRAME.a <= 0 through as its raw rgb, which is black.  The calls below render one phase of a regular lattice (a quarter of
 * the pixels at stride 2: four times the frames for the cost of one) and give every unrendered pixel a mean and a count taken from rendered
 * neighbours of the same surface, found through the feature records, which exist for every pixel at full resolution.  The guided filter then
 * runs unchanged.  Every call of the other headers stays exactly as it is; these are opt-in.  Nothing is written back into FRAME.
 *
 * Definitions.  Those of include/pt_denoise.h, include/pt_guided.h and include/pt_demod.h hold.  floor = the call's albedo_floor, 0 or finite
 * and > 0.  floor == 0 selects the PLAIN rule: x_q = c_q, the mean, and a_p = (1, 1, 1).  floor > 0 selects the DEMODULATED rule: x_q = I_q of
 * include/pt_demod.h (c_q / a_q on a valid hit, c_q on a miss), and a_p = (fmaxf(Kd.r, floor), fmaxf(Kd.g, floor), fmaxf(Kd.b, floor)) for a
 * hole that is a hit, (1, 1, 1) for a hole that is a miss.  A pixel is a hit when its hit code (F1.w as an integer) is >= 0, else a miss, as
 * include/pt_denoise.h classes it.  A_q = FRAME.a of q.
 *   Hole.  A pixel p with FRAME.a <= 0 whose t, N and Kd (F0 and F1.rgb) are finite.  A pixel with FRAME.a > 0 is never changed, and a NaN
 *   FRAME.a is not a hole.
 *   Source.  A tap q = p + (dx, dy), dx, dy in -2 .. 2 at unit step, taps in row-major order (dy outer), p itself excluded, that
 *     - is in the image;
 *     - is valid as include/pt_denoise.h defines it (under the demodulated rule: and its I_q is finite, as include/pt_demod.h asks);
 *     - is a hit when p is a hit, a miss when p is a miss;
 *     - for a hit, has p's material (F2.w).
 *   Weight.  h = [1,4,6,4,1]/16, sn, sd, sa the call's sigma_normal, sigma_depth, sigma_albedo, each 1/sigma^2 clamped to FLT_MAX (+inf = off):
 *     hit:   w = h(dx) h(dy) exp(-(|N_p - N_q|^2 / sn^2 + ((t_p - t_q) / t_p)^2 / sd^2 + |Kd_p - Kd_q|^2 / sa^2))
 *     miss:  w = h(dx) h(dy)
 *     a tap with w < 1e-30 is skipped.
 *   Result.  Over the sources that are not skipped: S = sum w, x'_p = sum w x_q / S per component, B = sum w^2 / A_q, A'_p = (S * S) / B: the
 *   count of frames whose mean has the variance of x'_p when the sources are independent (k equal-weight sources of count A give k * A).
 *     FRAME'_p = ((a_p.r * x'_p.r) * A'_p, (a_p.g * x'_p.g) * A'_p, (a_p.b * x'_p.b) * A'_p, A'_p).
 *   A hole without such a source stays as it is, and FRAME' = FRAME bit for bit on every pixel that is no hole.  T is not changed: a filled hole
 *   has n = 0 < min_frames, so the filter pools its s2 over its window and takes v = s2 / A'_p.
 *
 * Filtered image.  pt_denoise_guided's rule (floor == 0) or pt_denoise_guided_demod's (floor > 0) word for word on (FRAME', T); the
 * output alpha is the real FRAME.a, so a == 0 marks a reconstructed pixel.  Under the demodulated rule a filled pixel gets its own texel back:
 * x' is illumination, and a_p is the hole's own albedo.
 * Not under the bit-exact contract of the render path, as the filters are not (__expf, the device's summation order); a float32 model of the
 * text above agrees to about 1e-4 relative.  Which holes are filled is exact unless a weight lies at the 1e-30 cut.
 */
#ifndef PT_FILL_H
#define PT_FILL_H
#include "pt_api.h"
#ifdef __cplusplus
extern "C" {
#endif

/* pt_render_mask (include/pt_steer.h) with the mask of the pixels x % stride == phase_x && y % stride == phase_y (x, y in FRAME order), built
 * on the device: FRAME, T and *n_active (may be NULL) are bit for bit those of pt_render_mask with that mask.  stride 1 renders every pixel.
 * Errors as pt_render_mask; also PT_ERR_ARG: stride outside 1 .. 8, a phase outside 0 .. stride - 1. */
int pt_render_interleaved(pt_ctx* ctx, int first_frame, int n_frames, const int32_t* seeds, int stride, int phase_x, int phase_y, int64_t* n_active);
/* FRAME' of the current image into rgba_out[W*H*4], FRAME order; *n_filled (may be NULL) = the number of holes that found a source.  FRAME and T
 * are not modified.  Computes the feature records first if they are stale (see pt_read_features).  Synchronous.
 * PT_ERR_ARG: a null context or rgba_out, a sigma that is NaN or <= 0, albedo_floor NaN, negative or +inf.  PT_ERR_UNSUPPORTED: a context that
 * holds only part of the image (pt_create with shard_count > 1, a pt_create_multi_part group). */
int pt_fill_frame(pt_ctx* ctx, float sigma_normal, float sigma_depth, float sigma_albedo, float albedo_floor, float* rgba_out, int64_t* n_filled);
/* The filtered image above into rgba_out[W*H*4] (rgb = filtered colour, a = FRAME.a), FRAME order.  FRAME and T are not modified.  Synchronous.
 * Errors as pt_denoise_guided_demod (T never allocated included), except that albedo_floor == 0 is legal and selects the plain rule. */
int pt_denoise_guided_filled(pt_ctx* ctx, int iterations, float sigma_lum, float sigma_normal, float sigma_depth, float sigma_albedo, int min_frames,
                             float albedo_floor, float* rgba_out);
/* The same image converted to 8-bit exactly as pt_read_display converts a mean: rgb_out[W*H*3].  Errors as pt_denoise_guided_filled. */
int pt_read_display_denoised_guided_filled(pt_ctx* ctx, int iterations, float sigma_lum, float sigma_normal, float sigma_depth, float sigma_albedo,
                                           int min_frames, float albedo_floor, int java_bytes, uint8_t* rgb_out);

#ifdef __cplusplus
}
#endif
#endif
