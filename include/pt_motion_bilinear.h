/* include/pt_motion_bilinear.h — carry the accumulated image across moved and deformed geometry with bilinear taps, on top of
 * include/pt_motion.h (the mark, P' and N~) and include/pt_reproject_bilinear.h (the taps and their rule struct), libpt_hip.so.
 *
 * No reference counterpart.  pt_reproject_frame_moved hands each new pixel the history of ONE old pixel, (int)sy*W + (int)sx.  An animated
 * scene that moves by a fraction of a pixel per step has its history snapped by up to half a pixel on every carry: the moving object's edges
 * wander, and a pixel whose nearest old neighbour fails the tests restarts although a neighbour one pixel away would have passed.
 * pt_reproject_frame_moved_bilinear blends the qualifying old pixels around the projected point instead.  Every call of the other headers stays
 * exactly as it is; this one is opt-in.  The mark is include/pt_motion.h's pt_motion_mark, with its caller contract.
 *
 * Mapping.  Plain binary32 * + - / sqrt in the written order, no contraction.  Per new pixel p:
 *   1.-4. Steps 1 to 4 of include/pt_motion.h, word for word: step 1 is include/pt_reproject.h's overlay test; step 2 is include/pt_motion.h's
 *      hit / miss split with P' (where the hit's surface point was at the mark) and N~ (the normal it had there) and all of its rejections
 *      (a triangle or ellipsoid id beyond either count, den not finite or <= 0, P' or N~ not finite, a moved ellipsoid with a rotation, any
 *      other type), v = P' - O' for a hit and v = D for a miss; steps 3 and 4 go through sx, sy and their range test.
 *   5.-9. Steps 5 to 9 of include/pt_reproject_bilinear.h, word for word, with two substitutions.  Rh is the mark's.  A tap's step-5 test
 *      uses |v| of P' and N~ in place of N; the material test is unchanged.  With albedo_floor > 0 the ratios use b_n[p] from Rn as it stands
 *      and b_h[s_k] from the mark's Rh.
 * With no primitive moved the result is pt_reproject_frame_bilinear's bit for bit.  A pixel with exactly one counting tap is the bit-exact
 * copy that pt_reproject_frame_moved makes.  (int)sx, (int)sy is always one of the four taps with a weight of at least 0.25, or the tap snapped
 * to: every pixel pt_reproject_frame_moved keeps is kept here.  With the camera fixed, a pixel on an unmoved primitive projects onto its own
 * centre and has one tap (step 7): it is pt_reproject_frame_moved's, bit for bit.
 *
 * Caller notes.  As include/pt_reproject_bilinear.h's: continue with frame numbers other than 1, and show the image with pt_read_display_mean
 * (include/pt_adaptive.h), not pt_read_display.  The counts FRAME.a and T.n of a blended pixel are weighted means of its taps' counts and so
 * no longer whole numbers; every call that reads them takes them as floats.
 * Out of scope: bilinear taps for pt_reproject_frame_through, a wider search when no tap counts, higher-order kernels, and what
 * include/pt_motion.h excludes (a changed topology; lighting that changes away from the moved object).
 */
#ifndef PT_MOTION_BILINEAR_H
#define PT_MOTION_BILINEAR_H
#include "pt_motion.h"
#include "pt_reproject_bilinear.h"
#ifdef __cplusplus
extern "C" {
#endif

/* pt_reproject_frame_moved with the mapping above: replaces the current image's FRAME, and T when it is allocated.  Completes all submitted
 * work first; synchronous.  Between the mark and the call the bindings pt_reproject_frame_moved names may be uploaded.  On success the current
 * inputs become the image's camera, recorded in the current scene, and the mark is spent.  *n_kept = the pixels that kept history,
 * *n_blended = those among them blended from two or more old pixels (either may be NULL).  Later renders are bit-identical to renders on top
 * of pt_write_frame (and pt_write_moments) of the result; one-stream and pt_create_multi contexts give identical results.  An image without
 * a camera and with no mark is left alone (PT_OK, both counts 0), as pt_reproject_frame_bilinear leaves it.
 * PT_ERR_ARG: null context or rule; snap outside [0, 0.5) or NaN; albedo_floor negative, NaN or infinite; max_history, depth_tol, normal_tol
 * or flags as pt_reproject_frame refuses them (the argument checks of pt_reproject_frame_bilinear, in its order, under this call's name);
 * then every case of pt_reproject_frame_moved: its Parameters, no mark, the mark of another image, the image's camera record no longer the
 * marked one, binding 14, binding 5 or a texture uploaded since the mark.
 * PT_ERR_UNSUPPORTED: as pt_reproject_frame_moved.  On every error FRAME, T and the mark are unchanged and both counts are 0. */
int pt_reproject_frame_moved_bilinear(pt_ctx* ctx, const pt_reproject_bilinear_rule* rule, int64_t* n_kept, int64_t* n_blended);

#ifdef __cplusplus
}
#endif
#endif
