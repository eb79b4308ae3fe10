/* include/pt_demod.h — albedo demodulation for the guided filter, its selection and the reprojection, on top of include/pt_api.h (libpt_hip.so),
 * include/pt_denoise.h (feature records, pixel classes), include/pt_guided.h (the filter), include/pt_steer.h (the rule) and
 * include/pt_reproject.h (the mapping).
 *
 * No reference counterpart.  The calls of those headers filter, compare and carry the COLOUR c = FRAME.rgb / FRAME.a.  trace() multiplies the
 * diffuse throughput by the first hit's Kd (frag.glsl:873), and with BLUR = 0 every sample of a pixel has the same first hit, so for a diffuse
 * first hit c = Kd * illumination exactly.  The calls below work on the ILLUMINATION c / Kd instead and put the pixel's own Kd back at the end:
 * a map_Kd texture is neither blurred by the filter nor an obstacle to it, the pooled moments of a textured surface measure noise and not the
 * texture's contrast, and a reprojected pixel keeps its own texel.  Every call of the other headers stays exactly as it is; these are opt-in.
 *
 * Definitions.  floor = the call's albedo_floor, finite and > 0.  Kd = F1.rgb of the pixel's feature record (Kd after mapMtl), l(c) =
 * (0.2126*c.r + 0.7152*c.g) + 0.0722*c.b as in include/pt_guided.h, c_p the mean of include/pt_denoise.h, T_p = (sY, sYY, n, 0).
 *   Filter-side albedo.  For a pixel that include/pt_denoise.h classes as a valid hit: a_p = (fmaxf(Kd.r, floor), fmaxf(Kd.g, floor),
 *   fmaxf(Kd.b, floor)), L_p = l(a_p), I_p = c_p / a_p per component.  A valid hit whose I_p has a non-finite component is treated as INVALID
 *   from here on (in the filter and in step 4 of the selection).  For a miss or an invalid pixel a_p = (1, 1, 1) and L_p = 1 by definition
 *   (not by evaluating l), so I_p = c_p and such pixels see exactly the plain rule.  T'_p = (sY / L_p, (sYY / L_p) / L_p, n, 0).
 *   l(c / a) = l(c) / l(a) holds for a grey albedo only; for a coloured one T' is an approximation of the illumination's luminance moments
 *   (the ratio of the two is the same for every frame of a pixel, so the relative noise is kept).
 *
 * Filter.  include/pt_guided.h's rule word for word on (I, T') in place of (c, T): the counts A = FRAME.a, the classes (apart from the pixels
 * made invalid above), the features, the pooling over the 7x7 window of the same class and material (each tap's moments divided by that tap's
 * own L) are unchanged, and the albedo edge term still compares the raw Kd (sigma_albedo = +inf switches it off, the natural setting here).
 * The result (I_K, v_K) gives the output rgb = a_p * I_K per component, a = FRAME.a.  Invalid pixels are passed through as include/pt_denoise.h
 * passes them.  iterations 0 gives a_p * (c_p / a_p), two correctly rounded operations: within 2 ulp of the mean, not bit-identical to it.
 * Like pt_denoise_guided not under the bit-exact contract (__expf, sqrtf, the device's summation order) but within the bound of
 * tests/_guided_ref64.py on I_K, times a_p, plus the rounding of the last product; nearly converged pixels as include/pt_guided.h says.
 *
 * Selection.  Steps 1-4 of include/pt_steer.h unchanged, on the raw T.  Step 5: c_K = a_p * I_K, tol = fmaxf(rel_err * fabsf(l(c_K)), abs_err),
 * active iff v_K == +inf or (v_K * L_p) * L_p > tol * tol; a NaN is inactive.  (v_K is a variance of illumination; L_p^2 brings it back to colour.)
 *
 * Reprojection.  Steps 1-6 of include/pt_reproject.h unchanged.  The albedos here have a rule of their own, because they are needed for pixels
 * the filter would class otherwise: b_n[p] = (fmaxf(Kd.r, floor), fmaxf(Kd.g, floor), fmaxf(Kd.b, floor)) of Rn[p] when Rn[p] is a hit (hit
 * code not -1, as there) whose Kd is finite, else (1, 1, 1); b_h[s] the same from Rh[s].  Step 7 for a kept pixel, F = FRAME[s], T = T[s]:
 *   r = b_n[p] / b_h[s] per component, rho = l(b_n[p]) / l(b_h[s]);
 *   F' = (F.r * r.r, F.g * r.g, F.b * r.b, F.a), then the cap exactly as there: F'.a > max_history gives (F'.r*f, F'.g*f, F'.b*f, max_history);
 *   T' = (sY * rho, (sYY * rho) * rho, n, 0), then T's own cap on n (the fourth component is carried as pt_reproject_frame carries it).
 *   F' and T' are not checked for finiteness again.
 * Plain binary32 in the written order without contraction: bit-exact against its model, like pt_reproject_frame.  The ratio form is
 * deliberate: with the camera unchanged s = p, r and rho are exactly 1, and the call is the identity wherever pt_reproject_frame is.
 */
#ifndef PT_DEMOD_H
#define PT_DEMOD_H
#include "pt_api.h"
#include "pt_steer.h"
#ifdef __cplusplus
extern "C" {
#endif

/* pt_denoise_guided on the illumination, as defined above.  Errors as pt_denoise_guided; also PT_ERR_ARG: albedo_floor not finite or not > 0. */
int pt_denoise_guided_demod(pt_ctx* ctx, int iterations, float sigma_lum, float sigma_normal, float sigma_depth, float sigma_albedo, int min_frames,
                            float albedo_floor, float* rgba_out);
/* The same image converted to 8-bit exactly as pt_read_display converts a mean: rgb_out[W*H*3].  Errors as pt_denoise_guided_demod. */
int pt_read_display_denoised_guided_demod(pt_ctx* ctx, int iterations, float sigma_lum, float sigma_normal, float sigma_depth, float sigma_albedo,
                                          int min_frames, float albedo_floor, int java_bytes, uint8_t* rgb_out);
/* pt_select_guided with the step 5 above.  FRAME and T are not modified.  Errors as pt_select_guided; also PT_ERR_ARG: albedo_floor not finite
 * or not > 0. */
int pt_select_guided_demod(pt_ctx* ctx, const pt_guided_rule* rule, float albedo_floor, uint8_t* mask_out, int64_t* n_active);
/* pt_select_guided_demod, then pt_render_mask on its mask: FRAME, T and *n_active are bit for bit those of the two calls made one after the
 * other.  Errors as pt_render_adaptive_guided; also PT_ERR_ARG: albedo_floor not finite or not > 0. */
int pt_render_adaptive_guided_demod(pt_ctx* ctx, int first_frame, int n_frames, const int32_t* seeds, const pt_guided_rule* rule, float albedo_floor,
                                    int64_t* n_active);
/* pt_reproject_frame with the step 7 above; flags as there.  Errors as pt_reproject_frame; also PT_ERR_ARG: albedo_floor not finite or not > 0.
 * On every error FRAME and T are unchanged. */
int pt_reproject_frame_demod(pt_ctx* ctx, float max_history, float depth_tol, float normal_tol, int flags, float albedo_floor, int64_t* n_kept);

#ifdef __cplusplus
}
#endif
#endif
