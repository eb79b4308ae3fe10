/* include/pt_reproject.h — carry the accumulated image across a camera move, on top of include/pt_api.h (libpt_hip.so).
 *
 * No reference counterpart: the reference resets FRAME on every frame in which the camera moves or has just stopped (dispatch.java:645-690,
 * resetTexture).  pt_reproject_frame instead hands every pixel of the new view the sum and count of the old pixel that saw the same surface
 * point, so that only disoccluded pixels start from zero.  Nothing else changes: no render path, kernel or other entry point.
 *
 * The image's camera.  The library records the frame inputs (ORIGIN, ROTATION, MOUSE_POS, Parameters) of each of the four ring images:
 * a render call (pt_render, pt_render_batch, pt_render_batch_async, pt_render_adaptive) records the inputs it renders with in the image it
 * is submitted for; pt_write_frame records the inputs current at the call; pt_reset_frame and pt_next_image leave the image with no camera.
 *
 * Mapping.  From the image's camera (') to the current frame inputs, per new pixel p, plain binary32 * + / sqrt in the written order (no
 * fused multiply-add).  M' = rotationMatrix(ROTATION') as k_frame_setup builds it (row-major, direction = q * M'), O' = ORIGIN',
 * ss', fl', hr' = screenSize', focalLength', screenHratio'.  Rn = the feature records of include/pt_denoise.h under the current inputs,
 * Rh = the same under the image's camera; FRAME and T (include/pt_adaptive.h, when allocated) are the image's.
 *   1. p under the current MOUSE_POS overlay (frag.glsl:888): 0 to FRAME and T.
 *   2. Rn[p] is a hit if its hit code is not -1, else a miss.  A hit is rejected if t, N or D is not finite, or if its material is
 *      view-dependent and flags lacks PT_REPROJECT_ALL_MATERIALS.  View-dependent: Pr != 1, Pc != 0, Tr > 0, Tf[0] > 0, illum 5 or 7,
 *      or a map_Pr, map_Pc or map_Tr >= 0 (what gives chooseRay, frag.glsl:745-809, a mirror, clearcoat or transmission lobe).
 *      Hit: P = O + t*D per component (O = ORIGIN), v = P - O'.  Miss: v = D (a point at infinity).
 *   3. q_i = (v0*M'[3i] + v1*M'[3i+1]) + v2*M'[3i+2]; rejected unless q2 > 0.
 *   4. a = (q0/q2)*fl', b = (q1/q2)*fl', sx = ((1 - a/ss')*0.5)*W, sy = ((1 + b/(hr'*ss'))*0.5)*H; rejected unless 0 <= sx < W and
 *      0 <= sy < H (NaN fails).  Source s = (int)sy*W + (int)sx: the nearest pixel, no blending, so sums and counts stay whole samples.
 *   5. Miss: Rh[s] must be a miss.  Hit: Rh[s] must be a hit of the same material with a finite t' > 0,
 *      |sqrt((v0*v0 + v1*v1) + v2*v2) - t'| <= depth_tol*t', and (N0*N0' + N1*N1') + N2*N2' >= normal_tol (normals before the
 *      face-forward flip, so independent of the view).
 *   6. F = FRAME[s]; rejected unless F.a > 0 and F.rgb is finite.
 *   7. Kept: FRAME[p] = F, or, when F.a > max_history, (F.r*f, F.g*f, F.b*f, max_history) with f = max_history / F.a; T[p] = T[s] under
 *      the same cap on its own n (sY and sYY scaled by max_history / n).  A rejected pixel gets 0 in FRAME and T.
 * With the camera unchanged the call is the identity on every pixel that is kept, apart from the cap.
 *
 * Caller notes.  A render with u_frameCount == 1 overwrites FRAME (frag.glsl:924-927, kept bit for bit): after a reprojection continue
 * with frame numbers other than 1.  Pixels now carry different counts: show the image with pt_read_display_mean (include/pt_adaptive.h),
 * not pt_read_display.
 */
#ifndef PT_REPROJECT_H
#define PT_REPROJECT_H
#include "pt_api.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PT_REPROJECT_ALL_MATERIALS 1   /* also reuse pixels whose first-hit material is view-dependent */

/* Replaces the current image's FRAME, and T when it is allocated, by the mapping above from the image's camera to the current frame inputs;
 * the current inputs then become the image's camera.  Completes all submitted work first, as pt_write_frame does.  An image without a
 * camera is left alone (PT_OK, *n_kept = 0).  *n_kept (may be NULL) = the pixels that kept their history.  Synchronous; later renders are
 * bit-identical to renders on top of pt_write_frame of the result.  One-stream and pt_create_multi contexts give identical results.
 * PT_ERR_ARG: null context; max_history not >= 1; depth_tol not > 0; normal_tol outside [-1, 1] or NaN; unknown flags bits; Parameters not
 * set or not matching the image size; a scene buffer (any binding but 0, 1, 2, 4) or a texture uploaded since the image's camera was recorded.
 * PT_ERR_UNSUPPORTED: Parameters.DEBUG != 0 (now or in the image's camera); a context that holds only part of the image (pt_create with
 * shard_count > 1, a pt_create_multi_part group).  On every error FRAME and T are unchanged. */
int pt_reproject_frame(pt_ctx* ctx, float max_history, float depth_tol, float normal_tol, int flags, int64_t* n_kept);

#ifdef __cplusplus
}
#endif
#endif
