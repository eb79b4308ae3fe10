/* include/pt_reproject_through.h — carry the history of mirror and glass pixels across a camera move, through their seen-through chains, on top
 * of include/pt_reproject.h and include/pt_through.h (libpt_hip.so).
 *
 * No reference counterpart.  pt_reproject_frame rejects every pixel whose first hit is view-dependent, and PT_REPROJECT_ALL_MATERIALS carries the
 * sphere's own surface point, which smears what is seen IN the sphere.  The seen-through record S of include/pt_through.h names the surface at
 * the end of a pixel's deterministic chain of delta lobes, and pt_read_through_rays the segment that found it: a world point, a normal and a
 * material.  Where that end surface is not view-dependent, the radiance it sends up the chain is the same from the old camera and the new one,
 * and this call hands the pixel the sum and count of the old pixel whose chain ended on the same point.  Every call of the other headers stays
 * exactly as it is; this one is opt-in.
 *
 * The rule.  Plain binary32 * + - / in the written order, no fused multiply-add.  Rn / Rh = the first-hit records of include/pt_denoise.h under
 * the current inputs / under the image's camera (include/pt_reproject.h); Sn / Sh and Yn / Yh = the seen-through records and their last
 * segments (pt_read_through_rays' layout: O, t, D, k) under `thru`, for the same two cameras; O = ORIGIN, and O', M', ss', fl', hr' the image's
 * camera as in include/pt_reproject.h; FRAME and T are the image's.  k_p = Sn[p].S3.z as an int.
 *   1. p under the current MOUSE_POS overlay: 0 to FRAME and T.
 *   2. k_p == 0: steps 2-7 of include/pt_reproject.h on Rn, Rh, word for word.  (With thru->max_depth == 0 or thru->lobes == 0 the whole call
 *      therefore equals pt_reproject_frame bit for bit.)
 *   3. k_p >= 1, a chain pixel.  Rejected unless Sn[p] is a hit (hit code not -1), its L is finite and > 0, its N and D0 are finite and O, t, D
 *      of Yn[p] are finite; unless the end surface's material, the low 12 bits of the surface word, is a material of the scene; and unless
 *      that material is not view-dependent (include/pt_reproject.h's definition), which flags & PT_REPROJECT_ALL_MATERIALS lifts.
 *      The end point: X = Yn.O + Yn.t * Yn.D per component.
 *   4. The guess.  The virtual point V = O + L * D0 per component (exact for a chain of planar mirrors, a starting point for anything else);
 *      v = V - O', then steps 3-4 of include/pt_reproject.h: rejected unless q2 > 0 and 0 <= sx < W and 0 <= sy < H; (cx, cy) = ((int)sx, (int)sy).
 *   5. The search.  Candidates s = (x, y), y from cy - radius to cy + radius (outer), x from cx - radius to cx + radius (inner), those outside
 *      the image skipped.  A candidate qualifies when Sh[s]'s surface word equals Sn[p]'s as an integer (with PT_THROUGH_KEY: k, the first-hit
 *      material and the end material at once); Sh[s] is a hit and X' = Yh.O + Yh.t * Yh.D is finite; with e = X' - X and
 *      d2 = (e0*e0 + e1*e1) + e2*e2, d2 <= (point_tol*L) * (point_tol*L); (N0*N0' + N1*N1') + N2*N2' >= normal_tol; and FRAME[s].a > 0 with a
 *      finite rgb.  A NaN fails every compare.  The source is the qualifying candidate of smallest d2, the first in search order on a tie; with
 *      none the pixel is rejected.
 *   6. Step 7 of include/pt_reproject.h from the source: the cap on max_history for FRAME, and for T on its own n.  A rejected pixel gets 0 in both.
 * With the camera unchanged the call is the identity on every pixel that is kept, apart from the cap (the guess is p itself, and X' == X there:
 * d2 = 0).  A chain pixel whose own FRAME cell has no history takes the nearest qualifying neighbour's, which no first-hit pixel does.
 *
 * Out of scope.  Moved geometry under a chain: the scene must be unchanged since the image's camera, as in pt_reproject_frame.  Demodulated
 * carry for chain pixels.  A chain that leaves into the sky: it keeps the mirror's own k = 0 record (include/pt_through.h) and is rejected as a
 * view-dependent first hit is today.  The share of a glass pixel that comes from the lobe the chain did not follow: it is carried as it is;
 * max_history and the history validation of include/pt_validate.h bound it.
 */
#ifndef PT_REPROJECT_THROUGH_H
#define PT_REPROJECT_THROUGH_H
#include "pt_reproject.h"
#include "pt_through.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pt_reproject_through_rule {
    float max_history, depth_tol, normal_tol;   /* include/pt_reproject.h's, for every pixel */
    float point_tol;                            /* chain pixels: |X' - X| <= point_tol * L */
    int   radius;                               /* 0 .. 4: the search window around the guess */
    int   flags;                                /* PT_REPROJECT_ALL_MATERIALS */
} pt_reproject_through_rule;

/* pt_reproject_frame with the rule above: replaces the current image's FRAME, and T when it is allocated; the current inputs then become the
 * image's camera, so that pt_history_hold (include/pt_validate.h) may follow.  *n_kept (may be NULL) = the pixels that kept their history,
 * *n_kept_through (may be NULL) = those among them with k_p >= 1.  An image without a camera is left alone (PT_OK, both counts 0).
 * Synchronous; one-stream and pt_create_multi contexts give identical results.
 * PT_ERR_ARG: a null context or rule; radius outside 0 .. 4; point_tol not > 0; a thru with max_depth > 0 and lobes != 0 but without
 * PT_THROUGH_KEY (the one integer compare of step 5 rests on the key); include/pt_through.h's errors for thru; everything pt_reproject_frame
 * reports for max_history, depth_tol, normal_tol, flags, the Parameters and uploads since the image's camera.
 * PT_ERR_UNSUPPORTED: as pt_reproject_frame; PT_THROUGH_KEY in a scene with more than 4096 materials.  On every error FRAME and T are unchanged. */
int pt_reproject_frame_through(pt_ctx* ctx, const pt_through_rule* thru, const pt_reproject_through_rule* rule, int64_t* n_kept,
                               int64_t* n_kept_through);

#ifdef __cplusplus
}
#endif
#endif
