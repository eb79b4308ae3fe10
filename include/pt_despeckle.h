/* include/pt_despeckle.h — outlier rejection: pull a firefly pixel back to the ceiling of its surface neighbourhood (libpt_hip.so).
 *
 * No reference counterpart: the reference accumulates whatever its samples return.  At low sample counts a path tracer with glass and metal
 * leaves single pixels whose mean is tens of times their neighbours', because one sample found a caustic path.  Every image-space consumer
 * treats such a pixel as signal: the guided filter spreads it (its own variance is huge, so its luminance term is loose), the reprojections
 * carry it until max_history ages it out, pt_history_merge sees it as disagreement and the steering rule keeps sampling around it.  The two
 * calls here are the neighbourhood clamp that SVGF-style pipelines put in front of the filter, built from what the library already has: the
 * feature records say which neighbours lie on the same surface, and T says whether a pixel's excess is explainable by its own noise.
 * Nothing else changes: no render path, kernel or other entry point.
 *
 * The rule.  Binary32 + - * / sqrt in the written order, no fused multiply-add.  max(x, 0) is include/pt_guided.h's: x for x >= 0, 0 for
 * x < 0, +inf for NaN.  A_q = FRAME[q].a;  c_q = FRAME[q].rgb / A_q (three divisions);  l_q = (0.2126*c.r + 0.7152*c.g) + 0.0722*c.b.
 * q is measured iff A_q > 0 and l_q is finite.  R = the feature records of include/pt_denoise.h under the current inputs (F0 = (t, N),
 * F1.w = the hit code, F2.w = the material word); r = rule.radius.  For every pixel p:
 *   1. p is unchanged (s = 1) if it lies under the current MOUSE_POS overlay or is not measured.
 *   2. Window: the taps q = p + (dx, dy), dy outer and dx inner, both from -r to r, q != p.  A tap counts iff all of
 *        - it lies in the image;
 *        - it is measured;
 *        - it has p's class (hit iff the hit code is not -1);
 *        - for a hit, it has p's material word (F2.w, compared as integers);
 *        - for a hit, (N_p.x*N_q.x + N_p.y*N_q.y) + N_p.z*N_q.z >= normal_tol (a NaN fails).
 *      Over the counting taps, in that order, from 0:  K = sum 1,  S = sum l_q,  Q = sum l_q*l_q.
 *   3. K < min_taps: unchanged.
 *   4. mu = S/K,  s2 = max((Q - S*mu)/(K - 1), 0),  hi = mu + sigmas*sqrt(s2);  if hi < min_lum then hi = min_lum.
 *      Unless l_p > hi: unchanged.  (A NaN or infinite hi therefore changes nothing.)
 *   5. If own_z is finite and T_p.n >= 2:  m = sY/n,  s2p = max((sYY - sY*m)/(n - 1), 0),  v = s2p/A_p,  d = l_p - mu;
 *      unchanged if d*d > (own_z*own_z)*v.  A NaN on either side does not make the comparison true: the pixel is clamped.  n < 2 is no
 *      estimate and the test passes.  This step keeps a converged one-pixel highlight — its deviation is many standard errors of its own
 *      mean — and clamps a spike: one sample of 1000 among 16 frames deviates by about one of its own standard errors.
 *   6. s = hi/l_p.  FRAME'[p] = (rgb*s per component, a unchanged);  T'[p] (when T is allocated) = (sY*s, sYY*(s*s), n, 0);
 *      scale_out[p] = s;  the pixel counts in n_clamped.
 * An unchanged pixel keeps FRAME[p] and T[p] bit for bit and has scale_out[p] = 1.  Every tap reads the original image: the result depends
 * on no order, and one pass is the whole rule.
 *
 * Biases, all deliberate.  The call REMOVES ENERGY: what it takes off a caustic's rare bright samples is not given to any other pixel, so
 * the expected image is darker than the converged one wherever such paths carry light; own_z limits this to pixels whose excess is
 * statistically unsupported, and min_lum keeps dark regions out of it.  pt_despeckle_frame is IRREVERSIBLE: FRAME and T are overwritten,
 * and frames accumulated afterwards add to the clamped sums (use pt_despeckle to look first).  TWO ADJACENT FIREFLIES PROTECT EACH OTHER:
 * each is a tap of the other, raises mu and sigma of its window, and with few taps neither may exceed the ceiling; a larger radius dilutes
 * this, a second call does not mend it for pixels the first left unchanged.
 */
#ifndef PT_DESPECKLE_H
#define PT_DESPECKLE_H
#include "pt_api.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int   radius;      /* the window is (2*radius + 1)^2 pixels, the centre excluded; 1 .. 3 */
    float sigmas;      /* k: the ceiling is mu + k*sigma of the neighbours' mean luminances; finite, >= 0 */
    int   min_taps;    /* with fewer counting neighbours the pixel is left alone; 2 .. (2*radius + 1)^2 - 1 */
    float own_z;       /* the pixel's excess must be explainable by its own noise: d*d <= own_z^2 * v_p; > 0, +inf = the test is off (no T needed) */
    float normal_tol;  /* the window's normal test, [-1, 1] */
    float min_lum;     /* no ceiling lies below this luminance; finite, >= 0 */
} pt_despeckle_rule;

/* The rule above over the current image, read only: rgba_out[W*H*4] = (the rule applied to the mean: c_p*s per component; a = FRAME.a),
 * pt_denoise_guided's output convention, FRAME order; scale_out[W*H] = s; *n_clamped = the pixels clamped.  Each of the three may be
 * NULL.  Completes work in flight first.  FRAME, T, the image's camera record and the record caches' contents stay as they are.
 * PT_ERR_ARG: null context or rule; a field outside the range given above (a NaN is always outside), in the struct's order; Parameters /
 * ORIGIN / ROTATION not set, or Parameters that do not match the image size; own_z finite while T was never allocated.
 * PT_ERR_UNSUPPORTED: a context that holds only part of the image; Parameters.DEBUG != 0.  On every error *n_clamped is 0. */
int pt_despeckle(pt_ctx* ctx, const pt_despeckle_rule* rule, float* rgba_out, float* scale_out, int64_t* n_clamped);

/* Replaces FRAME (and T, when allocated) of the current image by the rule above, on every stream.  The image keeps its camera: the current
 * inputs, recorded again.  After it every consumer — the filters, demodulation, steering, fill, the reprojections, hold / merge and the
 * display — sees the clamped image.  One-stream and pt_create_multi contexts give identical results.  The same refusals; on every error
 * FRAME and T are unchanged. */
int pt_despeckle_frame(pt_ctx* ctx, const pt_despeckle_rule* rule, float* scale_out, int64_t* n_clamped);

#ifdef __cplusplus
}
#endif
#endif
