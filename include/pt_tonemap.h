/* include/pt_tonemap.h — the display image: metered exposure, a tone curve and the sRGB transfer, on the GPU (libpt_hip.so).
 *
 * No reference counterpart: the reference's screenshot path — pt_read_display — clamps FRAME.rgb / count to [0, 1] and rounds to 8 bits.  A
 * scene whose signal lies above 1 or far below it (emitters seen in glass and metal, a room lit by one small light) is white or black
 * there, and a caller who wants a viewable picture has had to read the float image back and map it on the host.  pt_tonemap does that
 * mapping where the image is, for every image the library produces: the current FRAME, or a host image in pt_denoise_guided's output
 * convention (what pt_denoise*, pt_denoise_guided*, pt_despeckle and pt_fill_frame deliver, or anything the caller computed).  Nothing else
 * changes: no render path, kernel or other entry point.
 *
 * The rule.  Binary32 + - * / in the written order, no fused multiply-add, no transcendental function.  For every pixel p: A = FRAME[p].a
 * and c = FRAME[p].rgb / A (three divisions); for a given image c = rgba_in[p].rgb as it is and A = rgba_in[p].a.
 *   1. Luminance.  l = (0.2126*c.r + 0.7152*c.g) + 0.0722*c.b.  p is metered iff A > 0, l is finite and l > 0.
 *   2. Histogram.  16 bins per octave, read off the float's bits: b = clamp((bits(l) >> 19) - 1776, 0, 511); 1776 = (127 - 16) << 4, so bin 0
 *      starts at 2^-16 and bin 511 ends at 2^16; anything below (denormals included) counts in bin 0, anything above in bin 511.  hist[b] =
 *      the metered pixels of bin b, 32-bit integers: the result depends on no order.  mid[b] = the float with the bits
 *      ((b + 1776) << 19) | (1 << 18), the middle of bin b.
 *   3. Metered exposure (rule.exposure == 0), on the host in binary64, in this order:  N = sum hist;  cut_lo = floor((double)lo_pct * N),
 *      cut_hi = floor((1.0 - (double)hi_pct) * N);  keep_b = how many of bin b's ranks cum_b .. cum_b + hist[b] lie in [cut_lo, N - cut_hi);
 *      K = sum keep_b;  S = sum (double)keep_b * (double)mid[b] in ascending b;  target = (double)key / (S / K), clamped to [min_exposure,
 *      max_exposure].  With N == 0 — or K == 0, which needs hi_pct - lo_pct below binary64's resolution at 1 — target = 1.0, clamped the
 *      same way.  e = target, or with prev_exposure > 0:  e = prev + (double)adapt * (target - prev).  The exposure is (float)e.
 *      With rule.exposure > 0 the exposure is that value, and the histogram is taken only if hist_out is given.
 *      The trimmed mean is arithmetic, over bin middles: a geometric mean (the usual "log-average") needs log and exp, which differ between
 *      a GPU, numpy and a libm; the bins are logarithmic already, so the trim does what the logarithm is wanted for — it keeps a few
 *      very bright pixels from setting the exposure.
 *   4. Apply, per channel.  A pixel with A <= 0 or a NaN A is black (0, 0, 0).  x = c * e;  a NaN becomes 0, x < 0 becomes 0 and
 *      x > 65504 becomes 65504 (an infinite sample shows white, not the NaN the curves would make of it).
 *        curve 0:  t = x
 *        curve 1:  t = (x * (1 + x/(white*white))) / (1 + x)                          (extended Reinhard)
 *        curve 2:  t = (x*(2.51f*x + 0.03f)) / (x*(2.43f*x + 0.59f) + 0.14f)          (the rational ACES fit)
 *      Then t is clamped to [0, 1]; a NaN t (0/0 in curve 1, when white*white underflows to 0) becomes 0.
 *   5. Transfer.  0: q = floor(t*255 + 0.5), pt_read_display's rounding.  1: q = the number of k in 1 .. 255 with t >= T[k], where T[k] is
 *      the smallest binary32 whose sRGB encoding (12.92 t up to 0.0031308, 1.055 t^(1/2.4) - 0.055 above, in binary64) times 255 reaches
 *      k - 0.5, and T[0] = 0: the sRGB code rounded correctly to 8 bits.  T is a constant of the library (scripts/tonemap_srgb_table.py
 *      generates it; pt_tonemap_srgb_thresholds returns it).
 *
 * What the call is not: no bloom, no local or bilateral operator, no java_bytes packing, no JNI native.  The defaults of the Python layer
 * (curve 2, transfer 1, key 0.18, the 10 % .. 95 % ranks, exposure within 2^-10 .. 2^10, white 4, adapt 1) are PROVISIONAL: common
 * choices, not tuned on this project's workloads.
 */
#ifndef PT_TONEMAP_H
#define PT_TONEMAP_H
#include "pt_api.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int   curve;         /* 0 none, 1 extended Reinhard, 2 the rational ACES fit */
    int   transfer;      /* 0 linear: floor(t*255 + 0.5) as pt_read_display; 1 sRGB through the threshold table */
    float exposure;      /* > 0: this multiplier; 0: metered from the histogram; finite, >= 0 */
    float key;           /* metered: the luminance the metered mean is mapped to; finite, > 0 */
    float lo_pct, hi_pct;/* metered: ranks below lo_pct*N and from hi_pct*N on are left out; 0 <= lo_pct < hi_pct <= 1 */
    float min_exposure, max_exposure; /* metered: the target is clamped to this; finite, 0 < min <= max */
    float white;         /* curve 1: the exposed value that maps to 1; finite, > 0 */
    float adapt;         /* metered, with prev_exposure > 0: e = prev + adapt*(target - prev); (0, 1] */
} pt_tonemap_rule;

enum { PT_TONEMAP_BINS = 512 };

/* The rule above over the current FRAME (rgba_in == NULL) or over rgba_in[W*H*4] (host, RGBA32F, FRAME order: rgb a mean, a = FRAME.a).
 * rgb_out[W*H*3]: the bytes, top row first (pt_read_display's layout without java_bytes);  *exposure_out: the exposure applied;
 * hist_out[PT_TONEMAP_BINS]: the histogram (taken whenever hist_out is given, also under a fixed exposure).  Each of the three may be
 * NULL.  prev_exposure: 0, or the exposure of the previous call, towards which rule.adapt damps the metered one.
 * Read only, stateless and synchronous: completes work in flight first; FRAME, T, the image's camera record and the record caches stay as
 * they are.  Needs no Parameters, ORIGIN or scene.  One-stream and pt_create_multi contexts give identical results.
 * Every field of the rule is checked on every call, whichever mode uses it.
 * PT_ERR_ARG: null context or rule; a field outside the range given above (a NaN is always outside), in the struct's order; prev_exposure
 * negative, NaN or infinite.  PT_ERR_UNSUPPORTED: a context that holds only part of the image.  On every error no output is written. */
int pt_tonemap(pt_ctx* ctx, const pt_tonemap_rule* rule, const float* rgba_in, float prev_exposure,
               uint8_t* rgb_out, float* exposure_out, uint32_t* hist_out);

/* The same image written as an 8-bit RGB PNG (pt_save_png's encoder).  The same refusals, and PT_ERR_ARG for a null path or a file that
 * cannot be written; on every error *exposure_out is not written. */
int pt_tonemap_save_png(pt_ctx* ctx, const pt_tonemap_rule* rule, const float* rgba_in, float prev_exposure,
                        const char* path, float* exposure_out);

/* T of step 5 into out[256].  Needs no device.  PT_ERR_ARG: null out. */
int pt_tonemap_srgb_thresholds(float out[256]);

#ifdef __cplusplus
}
#endif
#endif
