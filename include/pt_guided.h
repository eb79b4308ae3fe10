/* include/pt_guided.h — luminance moments for every render path and a variance-guided denoised image, on top of include/pt_api.h
 * (libpt_hip.so), include/pt_adaptive.h (T) and include/pt_denoise.h (feature records, the a-trous filter).
 *
 * No reference counterpart.  Together with pt_reproject_frame (include/pt_reproject.h), which carries FRAME and T across a camera move, the
 * two surfaces below make the loop of spatiotemporal variance-guided filtering (Schied et al. 2017): move, reproject, render k frames, filter
 * with each pixel's own noise.  Converged pixels pass almost untouched; pixels with little history are filtered hard.
 *
 * Moments.  T = (sY, sYY, n, 0) per accumulator slot, as include/pt_adaptive.h defines it.  While recording is on (pt_record_moments), every
 * frame that pt_render / pt_render_batch / pt_render_batch_async adds to FRAME also adds Y = (0.2126*r + 0.7152*g) + 0.0722*b of its colour
 * to T, in u_frameCount order, float32 without contraction: T += (Y, Y*Y, 1, 0), except that a frame with u_frameCount == 1 restarts T at
 * (Y, Y*Y, 1, 0) as it restarts FRAME.  So T.n == FRAME.a for every pixel whose frames were all recorded.  Mouse-overlay pixels and
 * DEBUG != 0 frames leave T alone, and so do frames that land in an earlier ring image after pt_next_image (T describes the current image).
 * FRAME is bit for bit what it is with recording off.  pt_render_adaptive keeps its own rule.
 *
 * Guided filter.  The definitions of include/pt_denoise.h hold unchanged: the pixel classes (invalid, hit, miss), the mean c_p = FRAME.rgb /
 * FRAME.a, the pass-through of invalid pixels (their mean, or their raw rgb when FRAME.a <= 0), taps outside the image or of another class
 * skipped, and the normal, depth and albedo terms with their sigmas (+inf = off, each 1/sigma^2 clamped to FLT_MAX; between two miss pixels
 * none of them counts).  Notation: l(c) = (0.2126*c.r + 0.7152*c.g) + 0.0722*c.b, A_p = FRAME.a, T_p = (sY, sYY, n).
 *   Per-frame variance s2_p of a valid pixel:
 *     n_p >= min_frames:  m = sY / n,  s2 = max((sYY - sY*m) / (n - 1), 0);
 *     otherwise pooled over the 7x7 window at unit step around p (p included, taps in row-major order): over the valid in-image taps q of
 *     p's class with n_q >= 1 (for a hit, also of p's material, F2.w), S = sum sY, Q = sum sYY, N = sum n (float32, in that order);
 *     N >= 2:  s2 = max((Q - S*(S/N)) / (N - 1), 0);  otherwise s2 = +inf (no estimate).
 *     max(x, 0) is x for x >= 0, 0 for x < 0, and +inf for a NaN x (no estimate).
 *   Variance of the mean: v_p = s2_p / A_p (A, not n: a pixel whose early frames were rendered before recording started is still right).
 *   Pass i = 0 .. K-1 (K = iterations), step s = 2^i, the 5x5 B3 taps h = [1,4,6,4,1]/16 at q = p + s*(dx, dy), dx, dy in -2 .. 2; the input
 *   (c, v) of pass i is the output of pass i-1:
 *     g_p  = sum k(dx) k(dy) v_q / sum k(dx) k(dy) over the 3x3 taps at unit step (valid, in-image, p's class), k = (1/4, 1/2, 1/4);
 *            g_p = +inf when one of those v_q is +inf
 *     e_c  = |l(c_p) - l(c_q)| / (sigma_lum * sqrt(g_p) + 1e-10), and 0 when sigma_lum is +inf or g_p is +inf
 *     w    = h(dx) h(dy) exp(-(e_c + |N_p - N_q|^2 / sn^2 + ((t_p - t_q) / t_p)^2 / sd^2 + |Kd_p - Kd_q|^2 / sa^2))   (hit; miss: e_c only);
 *            a tap with w < 1e-30 is skipped (so that where the exponential underflows is no part of the rule)
 *     c'_p = sum w c_q / sum w
 *     v'_p = sum w^2 v_q / (sum w)^2, and +inf when a tap that is not skipped has v_q = +inf
 *   Output: (c_K, FRAME.a) per pixel.  iterations 0 is the identity (the mean).
 * Not under the bit-exact contract of the render path, as pt_denoise: the device uses __expf and sqrtf and sums in its own order.  What it is
 * held to instead is the per-pixel bound that tests/_guided_ref64.py derives against a float64 evaluation of the text above: a few hundred
 * 2^-24 of the colours a pixel's passes reach where the filter is well conditioned.  A nearly converged pixel is not: sqrt(g_p) is small there,
 * a rounding of l(c) of a few 2^-24 moves e_c by 1e-3 and more, and the error compounds from pass to pass; the bound follows that, up to the
 * spread of the taps the pixel may take, and is no promise of 1e-4 there.
 */
#ifndef PT_GUIDED_H
#define PT_GUIDED_H
#include "pt_api.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Switches moment recording on (on != 0) or off for every stream of the context (a pt_create_multi / pt_create_multi_part group included).
 * Work in flight is completed first, under the previous setting.  Switching on allocates T zeroed where it is not allocated yet.  Default off.
 * PT_ERR_ARG: null context. */
int pt_record_moments(pt_ctx* ctx, int on);
/* T of the current image in FRAME's pixel order: out[W*H*4] = (sY, sYY, n, 0) per pixel; zeros when T was never allocated.  Completes work
 * in flight first.  pt_write_frame zeroes T, so a saved session is restored with pt_write_frame, then pt_write_moments.
 * PT_ERR_ARG: null pointer.  PT_ERR_UNSUPPORTED: a context that holds only part of the image (pt_create with shard_count > 1, a
 * pt_create_multi_part group). */
int pt_read_moments(pt_ctx* ctx, float* out);
/* Replaces T of the current image by in[W*H*4], FRAME's pixel order (allocating it if needed).  Completes work in flight first.
 * Errors as pt_read_moments. */
int pt_write_moments(pt_ctx* ctx, const float* in);
/* The guided filter above over the current image into rgba_out[W*H*4] (rgb = filtered mean, a = FRAME.a), FRAME order.  FRAME and T are not
 * modified.  Computes the feature records first if they are stale (see pt_read_features).  Synchronous.
 * PT_ERR_ARG: a null pointer, iterations outside 0 .. 8, min_frames < 2, a sigma that is NaN or <= 0, T never allocated (no moments: see
 * pt_record_moments).  PT_ERR_UNSUPPORTED: a context that holds only part of the image. */
int pt_denoise_guided(pt_ctx* ctx, int iterations, float sigma_lum, float sigma_normal, float sigma_depth, float sigma_albedo, int min_frames,
                      float* rgba_out);
/* The same image converted to 8-bit exactly as pt_read_display converts a mean (clamp, round, java_bytes, vertical flip): rgb_out[W*H*3].
 * Errors as pt_denoise_guided. */
int pt_read_display_denoised_guided(pt_ctx* ctx, int iterations, float sigma_lum, float sigma_normal, float sigma_depth, float sigma_albedo,
                                    int min_frames, int java_bytes, uint8_t* rgb_out);

#ifdef __cplusplus
}
#endif
#endif
