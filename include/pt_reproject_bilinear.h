/* include/pt_reproject_bilinear.h — carry the accumulated image across a camera move with bilinear taps, on top of include/pt_api.h
 * (libpt_hip.so), include/pt_reproject.h (the mapping) and include/pt_demod.h (the carried albedo).
 *
 * No reference counterpart.  pt_reproject_frame hands each new pixel the history of ONE old pixel, (int)sy*W + (int)sx.  Under a slow camera move
 * the projected point falls between old pixels, so the history is snapped by up to half a pixel on every call: edges wander, a dolly duplicates
 * or drops old pixels, and a pixel whose nearest old neighbour fails the depth, normal or material test restarts although a neighbour one pixel
 * away would have passed.  pt_reproject_frame_bilinear blends the qualifying old pixels around the projected point with bilinear weights instead
 * (the temporal accumulation of SVGF, Schied et al. 2017).  Every call of the other headers stays exactly as it is; this one is opt-in.
 *
 * Mapping.  The image's camera, Rn, Rh, FRAME and T are include/pt_reproject.h's, and so is the arithmetic: plain binary32 * + - / sqrt in the
 * written order, no contraction.  Per new pixel p:
 *   1.-4. Steps 1 to 4 of include/pt_reproject.h, word for word, through sx, sy and their range test (0 <= sx < W and 0 <= sy < H; NaN fails).
 *      The shader shoots through pixel centres (texCoord, frag.glsl:894), so a pixel's own ray projects to px + 0.5.
 *   5. The taps.  fx = sx - 0.5f, x0 = floorf(fx), wx = fx - x0.  Snapping: if wx < snap then wx = 0; else if wx > 1.0f - snap then x0 = x0 + 1
 *      and wx = 0.  The same in y gives y0 and wy.  ix = (int)x0, iy = (int)y0 (either may be -1).  The four taps are (ix + i, iy + j), j outer
 *      over 0, 1 and i inner over 0, 1, with weight w = ax_i * ay_j, ax_0 = 1.0f - wx, ax_1 = wx, and likewise ay.  A tap s COUNTS iff w > 0, it
 *      lies in the image, Rh[s] passes step 5 of include/pt_reproject.h against p's v, N and material (a miss against a miss; a hit against a
 *      hit of the same material within depth_tol and normal_tol), and FRAME[s] passes its step 6 (a > 0, finite rgb).  A NaN fails every compare.
 *   6. No counting tap: rejected, 0 to FRAME and T.
 *   7. Exactly one counting tap s: step 7 of include/pt_reproject.h from s (albedo_floor > 0: step 7 of include/pt_demod.h), T copied from s
 *      with its cap as those headers do.  With the camera unchanged, and for every pixel that has only its nearest neighbour, the call is
 *      therefore the bit-exact copy that pt_reproject_frame / pt_reproject_frame_demod make.
 *   8. Two or more counting taps.  Ws, A, C.rgb start at 0; per counting tap k in tap order, F = FRAME[s_k]: m = F.rgb / F.a per component; with
 *      albedo_floor > 0, m = m * r_k per component, r_k = b_n[p] / b_h[s_k] (b as in include/pt_demod.h); Ws = Ws + w, A = A + w * F.a,
 *      C = C + w * m.  Then mean = C / Ws, n = A / Ws, n' = n > max_history ? max_history : n, FRAME[p] = (mean.r*n', mean.g*n', mean.b*n', n').
 *   9. T, when allocated, of a pixel of step 8.  A tap enters iff it counts, T[s_k].n > 0 and sY and sYY are finite: y = sY / n, yy = sYY / n;
 *      with albedo_floor > 0, y = y * rho_k and yy = (yy * rho_k) * rho_k, rho_k = l(b_n[p]) / l(b_h[s_k]); WT = WT + w, NT = NT + w * n,
 *      Y = Y + w * y, YY = YY + w * yy, all from 0 in tap order.  No such tap: T[p] = 0.  Otherwise nT = NT / WT, capped at max_history as n is,
 *      and T[p] = ((Y / WT) * nT, (YY / WT) * nT, nT, 0).
 * (int)sx, (int)sy is always one of the four taps with a weight of at least 0.25, or the tap snapped to: every pixel pt_reproject_frame keeps
 * is kept here.
 *
 * Caller notes.  As include/pt_reproject.h's: continue with frame numbers other than 1, and show the image with pt_read_display_mean
 * (include/pt_adaptive.h), not pt_read_display.  The counts FRAME.a and T.n of a blended pixel are weighted means of its taps' counts and so
 * no longer whole numbers, as after the history merge of include/pt_validate.h; every call that reads them takes them as floats.
 * Out of scope: bilinear taps for pt_reproject_frame_through, a wider search when no tap counts, higher-order kernels.
 */
#ifndef PT_REPROJECT_BILINEAR_H
#define PT_REPROJECT_BILINEAR_H
#include "pt_api.h"
#include "pt_reproject.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_reproject_bilinear_rule {
    float max_history, depth_tol, normal_tol;   /* include/pt_reproject.h's */
    float snap;          /* [0, 0.5): a fractional offset closer than this to a pixel centre is that pixel */
    float albedo_floor;  /* 0: carry colour (pt_reproject.h step 7); finite > 0: carry illumination (pt_demod.h step 7) */
    int   flags;         /* PT_REPROJECT_ALL_MATERIALS */
} pt_reproject_bilinear_rule;

/* pt_reproject_frame with the mapping above: replaces the current image's FRAME, and T when it is allocated; the current inputs then become the
 * image's camera.  Completes all submitted work first; synchronous.  An image without a camera is left alone (PT_OK, both counts 0).
 * *n_kept = the pixels that kept history, *n_blended = those among them blended from two or more old pixels (either may be NULL).  Later renders
 * are bit-identical to renders on top of pt_write_frame (and pt_write_moments) of the result; one-stream and pt_create_multi contexts give
 * identical results.  PT_ERR_ARG and PT_ERR_UNSUPPORTED: every case of pt_reproject_frame; also PT_ERR_ARG: null rule; snap outside [0, 0.5) or
 * NaN; albedo_floor negative, NaN or infinite.  On every error FRAME and T are unchanged and both counts are 0. */
int pt_reproject_frame_bilinear(pt_ctx* ctx, const pt_reproject_bilinear_rule* rule, int64_t* n_kept, int64_t* n_blended);

#ifdef __cplusplus
}
#endif
#endif
