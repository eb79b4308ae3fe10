/* include/pt_validate.h — history validation: drop the carried samples that the new frames contradict (libpt_hip.so).
 *
 * No reference counterpart: the reference resets FRAME on any change.  The reprojections of include/pt_reproject.h and include/pt_motion.h
 * test geometry only (depth, normal, material), so lighting that changes away from a moved object — a moved shadow, a slid or dimmed light —
 * keeps its stale history until max_history ages it out, and an edit of an emitter's Ke (binding 14) cannot be carried at all.  The two calls
 * here keep the new frames apart from the history until the two have been compared: pt_history_hold moves FRAME and T aside, the caller
 * renders the new frames into the emptied image, pt_history_merge compares, per surface neighbourhood and in units of their noise, what the
 * new frames say with what the history says (the temporal-gradient test of adaptive SVGF, Schied et al. 2018), scales the history down where
 * the two disagree and adds it back.  Nothing else changes: no render path, kernel or other entry point.
 *
 * Caller contract.  The history held must describe the surfaces the new frames see, pixel by pixel.  An upload that moves no surface
 * (materials, binding 14; textures) needs nothing before the hold: hold, then render.  A camera move goes through pt_reproject_frame first, a
 * geometry move through pt_motion_mark / pt_reproject_frame_moved (a light is a quad in binding 3), then the hold.  The hold does not ask
 * that the scene is unchanged since the image's camera was recorded.  The new frames must all be rendered in one scene under one set of
 * frame inputs, which are still the current ones at the merge: the feature records R are computed under them.
 *
 * The hold.  On the device: H, the held FRAME, and V, the held T, W*H*16 B each, freed with the context; on the host the image's index, the
 * frame inputs of its camera record and the count of scene uploads.
 *
 * The rule.  Binary32 + - * / sqrt in the written order, no fused multiply-add.  max(x, 0) is include/pt_guided.h's: x for x >= 0, 0 for
 * x < 0, +inf for NaN.  N, U = FRAME and T now (the new frames); H, V = the held FRAME and T; R = the feature records of
 * include/pt_denoise.h under the current inputs in the current scene (F0 = (t, N), F1.w = the hit code, F2.w = the material word);
 * r = rule.radius.  For every pixel p:
 *   1. If p is under the current MOUSE_POS overlay, kappa = 1; go to 4.
 *   2. Window: the taps q = p + (dx, dy), dy outer and dx inner, both from -r to r, p included.  A tap counts iff all of
 *        - it lies in the image;
 *        - it has p's class (hit iff the hit code is not -1);
 *        - for a hit, it has p's material word (F2.w, compared as integers);
 *        - for a hit, (N_p.x*N_q.x + N_p.y*N_q.y) + N_p.z*N_q.z >= normal_tol (a NaN fails, for q = p too);
 *        - U_q.n >= 1 and V_q.n >= 1 (the tap is paired: both sides are summed over the same pixels, so that the surface's own spatial
 *          variation enters both means alike);
 *        - U_q.sY, U_q.sYY, V_q.sY and V_q.sYY are finite.
 *      Over the counting taps, in that order, from 0:
 *        SN = sum U.sY, QN = sum U.sYY, NN = sum U.n;   SH = sum V.sY, QH = sum V.sYY, NH = sum V.n.
 *   3. Unless NN >= 2 and NH >= 2: kappa = 1 (no evidence).  Otherwise
 *        mN = SN/NN, s2N = max((QN - SN*mN)/(NN - 1), 0);   mH = SH/NH, s2H = max((QH - SH*mH)/(NH - 1), 0)
 *        var = s2N/NN + s2H/NH,  d = |mN - mH|,  z = sqrt((d*d)/var)
 *        kappa = 1 when z is NaN or z <= z_lo;  0 when z >= z_hi;  else (z_hi - z)/(z_hi - z_lo).
 *   4. Merge, per component: FRAME'[p] = N[p] + kappa*H[p];  T'[p] = U[p] + kappa*V[p] in sY, sYY and n, and 0 in w.  With kappa == 0 exactly
 *      N and U (no multiply: an inf in H makes no NaN); with kappa == 1 exactly N + H and U + V.
 * A pixel that nothing was rendered into (pt_render_interleaved, a mask, an adaptive call) is no tap, but takes kappa from the rendered
 * taps of its window.  The count ignores max_history: the next reprojection caps it, as it does for plain accumulation.
 */
#ifndef PT_VALIDATE_H
#define PT_VALIDATE_H
#include "pt_api.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int radius;         /* the window is (2*radius + 1)^2 pixels; 1 .. 4 */
    float z_lo, z_hi;   /* the history is kept whole up to z_lo standard errors of disagreement and dropped from z_hi on */
    float normal_tol;   /* the window's normal test, [-1, 1] */
} pt_validate_rule;

/* Moves FRAME and T of the current image aside (H and V above) and zeroes both on every stream.  Completes all submitted work first.  The
 * image's camera record stays as it is (this is not pt_reset_frame).  A second hold replaces the first.
 * PT_ERR_ARG: null context; T was never allocated (pt_record_moments first); the current image has no camera.
 * PT_ERR_UNSUPPORTED: a context that holds only part of the image.  On every error FRAME, T and an earlier hold are unchanged. */
int pt_history_hold(pt_ctx* ctx);

/* Replaces FRAME and T of the current image by the rule above.  Completes work in flight first.  kappa_out (W*H floats, FRAME order) and
 * n_reduced (the pixels with H.a > 0 and kappa < 1) may be NULL.  On success the hold is spent and the current inputs are the image's camera.
 * Between the two calls any render entry point may run, with moment recording on, and pt_write_frame / pt_write_moments under the same
 * inputs.  One-stream and pt_create_multi contexts give identical results.
 * PT_ERR_ARG: null context or rule; radius outside 1 .. 4; z_lo or z_hi not finite, or not 0 <= z_lo < z_hi; normal_tol outside [-1, 1] or
 * NaN; no hold; the hold belongs to another image (pt_next_image); the image has no camera (pt_reset_frame); the image's camera record no
 * longer has the held frame inputs (a render or pt_write_frame under other inputs); a scene buffer or texture was uploaded since the hold;
 * Parameters that do not match the image size.
 * PT_ERR_UNSUPPORTED: Parameters.DEBUG != 0.  On every error FRAME, T and the hold are unchanged. */
int pt_history_merge(pt_ctx* ctx, const pt_validate_rule* rule, float* kappa_out, int64_t* n_reduced);

#ifdef __cplusplus
}
#endif
#endif
