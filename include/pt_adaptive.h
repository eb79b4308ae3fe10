/* include/pt_adaptive.h — adaptive sampling on top of include/pt_api.h (libpt_hip.so): render only the pixels that are still noisy.
 *
 * No reference counterpart: the reference traces every pixel every frame.  FRAME already keeps a per-pixel frame count in alpha
 * (frag.glsl:924-933), so an image whose pixels carry different counts is a legal FRAME; pt_read_display_mean shows it.
 *
 * Per-pixel statistics.  Every context keeps T = (sY, sYY, n, 0) per accumulator slot: the sum and the sum of squares of the luminance
 * Y = (0.2126*r + 0.7152*g) + 0.0722*b of the frames the pixel received from pt_render_adaptive (r, g, b = what the frame adds to FRAME),
 * and their number, all float32 without contraction.  T is allocated zeroed by the first pt_render_adaptive call and
 * zeroed again whenever FRAME is zeroed or replaced: pt_reset_frame, pt_write_frame, pt_next_image.  pt_render_adaptive always updates T;
 * frames rendered by pt_render / pt_render_batch / pt_render_batch_async go into FRAME, and into the statistics only while moment
 * recording is on (pt_record_moments, include/pt_guided.h).
 *
 * Selection, once per call before any frame is rendered; a pixel is active iff
 *   it is not under the mouse overlay, and not (max_frames > 0 && n >= max_frames), and
 *   n < min_frames, or err2 > tol*tol with
 *     mean = sY / n,  var = (sYY - sY*mean) / (n - 1),  err2 = var / n,  tol = fmaxf(rel_err * fabsf(mean), abs_err).
 * A NaN anywhere leaves the pixel inactive.  Every pixel-frame that is rendered is the reference's own job (rngState = pixel index +
 * u_seed), so an adaptive image is, pixel by pixel, bit-exactly what the selected frames give in the reference.
 */
#ifndef PT_ADAPTIVE_H
#define PT_ADAPTIVE_H
#include "pt_api.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Renders frames first_frame .. first_frame+n_frames-1 (seeds[i] = u_seed of frame first_frame+i) for the pixels that the selection
 * rule above marks active, and for no other pixel.  Synchronous, like pt_render_batch (batches still in flight are completed first,
 * into FRAME but not into the statistics).  *n_active (may be NULL) = the number of pixels rendered, summed over the context's streams.
 * PT_ERR_ARG: null context or seeds, n_frames < 1, min_frames < 2, max_frames < 0, rel_err / abs_err negative or NaN.
 * PT_ERR_UNSUPPORTED: Parameters.DEBUG != 0 (the heat map has no noise). */
int pt_render_adaptive(pt_ctx* ctx, int first_frame, int n_frames, const int32_t* seeds, float rel_err, float abs_err, int min_frames,
                       int max_frames, int64_t* n_active);
/* pt_read_display with every pixel divided by its own frame count (FRAME alpha) instead of one global frame_count; a pixel with
 * count 0 shows black.  Needs the whole image, like pt_read_display.  Synchronises. */
int pt_read_display_mean(pt_ctx* ctx, int java_bytes, uint8_t* rgb_out);

#ifdef __cplusplus
}
#endif
#endif
