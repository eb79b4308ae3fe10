/* include/pt_bloom.h — HDR glare ahead of the tone curve, and the display image of an image that stayed on the device (libpt_hip.so).
 *
 * No reference counterpart.  include/pt_tonemap.h maps a small emitter far above 1 to the same clipped white disc under every curve; the
 * glare around it is what tells a viewer how bright it is.  pt_bloom adds that glare to a float image — a bright pass, a pyramid of
 * ever coarser blurred copies, and their weighted sum laid back over the image — and pt_tonemap_bloom runs it between pt_tonemap's metering
 * and pt_tonemap's curve, all on the device.  Both take a third kind of source beside FRAME and a host image: the image the last filter
 * call left on the device, so that filter -> bloom -> display moves no float image through the host.  Nothing else changes: no render
 * path, no other entry point, and pt_tonemap's kernels run as they are.
 *
 * The rule.  Binary32 + - * / in the written order, no fused multiply-add, no transcendental function; every weight below is exact in
 * binary32.  Level 0 is the source, W_0 x H_0 = W x H; level k + 1 has W_(k+1) = (W_k + 1) / 2 and H_(k+1) = (H_k + 1) / 2 in integers: sizes
 * reach 1 and stay there, and no level count is refused for a small image.  L = rule.levels; clamp(i, 0, n - 1) below is "clamp".
 *   0. Source pixel.  c and A as in pt_tonemap: for FRAME, A = FRAME[p].a and c = FRAME[p].rgb / A (three divisions); for an image in the
 *      filter output convention c = rgb as it is and A = a.  The clean value s, per channel: a NaN becomes 0, c < 0 becomes 0, c > 65504
 *      becomes 65504.  A pixel with A <= 0 or a NaN A has s = (0, 0, 0): it emits no glare.
 *   1. Bright pass.  l = (0.2126*s.r + 0.7152*s.g) + 0.0722*s.b.  T = threshold / exposure, one binary32 division on the host.
 *      k = l > T ? (l - T) / l : 0.  B = s * k.
 *   2. Down.  D_(k+1)(x, y) is the separable tent (1, 3, 3, 1) / 8 = (0.125, 0.375, 0.375, 0.125) = w over the 4 x 4 texels
 *      p_ij = V_k(clamp(2x - 1 + i), clamp(2y - 1 + j)), with V_0 = B and V_k = D_k:  row_j = (w0*p_0j + w1*p_1j) + (w2*p_2j + w3*p_3j), and
 *      D_(k+1)(x, y) = (w0*row_0 + w1*row_1) + (w2*row_2 + w3*row_3).
 *   3. Up.  U_L = D_L.  For k = L - 1 .. 1:  U_k = D_k + spread * up(U_(k+1)), where for a texel (x, y) of the finer level
 *      cx = x >> 1, nx = clamp(cx + (x & 1 ? 1 : -1)), cy and ny likewise, and
 *      up(V)(x, y) = (0.5625*V(cx, cy) + 0.1875*V(nx, cy)) + (0.1875*V(cx, ny) + 0.0625*V(nx, ny)).
 *      G = up(U_1) * norm at the source's size, with norm = 1 / sum and sum computed on the host in binary32 as
 *      p = 1, sum = 1, then L - 1 times:  p = p * spread, sum = sum + p.   (A one-colour image under threshold 0 has G = its colour, up to
 *      rounding: the weights of every step sum to 1.)
 *   4. Compose.  out.rgb = c + intensity * G with the uncleaned c — a NaN pixel stays the pixel it was, and the tone mapper blacks it as
 *      before — and out.a = A.
 *
 * What the calls are not: no lens flare, no streaks, no anamorphic or spectral kernel, no local tone operator.  The glare is metered
 * on nothing: the exposure comes from the source image alone, so the histogram and the exposure are pt_tonemap's whatever the bloom rule.
 * The defaults of the Python layer (6 levels, intensity 0.05, threshold 1, spread 0.75) are PROVISIONAL: common choices, not tuned on
 * this project's workloads.
 */
#ifndef PT_BLOOM_H
#define PT_BLOOM_H
#include "pt_api.h"
#include "pt_tonemap.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int   levels;     /* 1 .. 8 pyramid levels */
    float intensity;  /* finite, >= 0: out = c + intensity * G */
    float threshold;  /* finite, >= 0, in exposed luminance: only light above threshold / exposure blooms */
    float spread;     /* finite, (0, 1]: weight of each coarser level relative to the next finer one */
} pt_bloom_rule;

/* The source image.  FRAME: the current FRAME, each pixel's rgb divided by its own count; rgba_in must be NULL.  HOST: rgba_in[W*H*4]
 * (host, RGBA32F, FRAME order: rgb a mean, a = FRAME.a), which must be given.  FILTERED: the image that the most recent successful
 * pt_denoise, pt_denoise_guided* or pt_read_display_denoised* call of this context left on the device, as it stands, with no copy through
 * the host; rgba_in must be NULL.  It is there from such a call until a call that uses that buffer for something else (today:
 * pt_select_guided* and pt_render_adaptive_guided* on an image without luminance moments, which zero it as their stand-in for T);
 * before the first, or after such an overwrite, the call is refused with PT_ERR_ARG. */
enum { PT_BLOOM_SRC_FRAME = 0, PT_BLOOM_SRC_HOST = 1, PT_BLOOM_SRC_FILTERED = 2 };
enum { PT_BLOOM_MAX_LEVELS = 8 };

/* Steps 0-4 into rgba_out[W*H*4] (host, RGBA32F, pt_denoise_guided's convention: rgb a mean, a the source's a).  exposure, positive and
 * finite, only scales the threshold.
 * All three calls are read only, stateless and synchronous: they complete work in flight first; FRAME, T, the image's camera record, the
 * record caches and the filtered image stay as they are.  One-stream and pt_create_multi contexts give identical results.
 * PT_ERR_ARG, in this order: null context; null rule; a field of the rule outside the range given above (a NaN is always outside), in the
 * struct's order; a source outside the enum; an rgba_in that does not fit the source; an exposure that is not positive and finite; then
 * PT_ERR_UNSUPPORTED for a context that holds only part of the image, and PT_ERR_ARG for a FILTERED source that is not there.
 * On every error no output is written. */
int pt_bloom(pt_ctx* ctx, const pt_bloom_rule* rule, int source, const float* rgba_in, float exposure, float* rgba_out);

/* pt_tonemap with the glare: steps 1-3 of pt_tonemap on the source image (exposure_out and hist_out are pt_tonemap's bit for bit, whatever
 * the bloom rule), the bloom under that exposure, then pt_tonemap's steps 4-5 on the composed image.  Outputs and prev_exposure as
 * pt_tonemap's.  The refusals: pt_tonemap's of the context, the tone-map rule and prev_exposure first, then pt_bloom's of the bloom rule,
 * the source and rgba_in. */
int pt_tonemap_bloom(pt_ctx* ctx, const pt_tonemap_rule* rule, const pt_bloom_rule* bloom, int source, const float* rgba_in,
                     float prev_exposure, uint8_t* rgb_out, float* exposure_out, uint32_t* hist_out);

/* The same image written as an 8-bit RGB PNG.  The same refusals, and PT_ERR_ARG for a null path or a file that cannot be written; on
 * every error *exposure_out is not written. */
int pt_tonemap_bloom_save_png(pt_ctx* ctx, const pt_tonemap_rule* rule, const pt_bloom_rule* bloom, int source, const float* rgba_in,
                              float prev_exposure, const char* path, float* exposure_out);

#ifdef __cplusplus
}
#endif
#endif
