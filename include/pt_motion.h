/* include/pt_motion.h — carry the accumulated image across moved and deformed geometry, on top of include/pt_reproject.h (libpt_hip.so).
 *
 * No reference counterpart: the reference resets FRAME on any change.  pt_reproject_frame (include/pt_reproject.h) refuses after any upload
 * of a scene buffer, so an edit to one object costs the whole accumulated image.  The two calls here let the caller move primitives in
 * between: pt_motion_mark remembers where every primitive was and what the image's camera saw, pt_reproject_frame_moved maps every pixel of
 * the current view, in the current scene, back to the old pixel that saw the same piece of surface.  No transform is passed: the library
 * compares the primitives' positions then and now.  Nothing else changes: no render path, kernel or other entry point; pt_reproject_frame
 * still refuses after any upload.
 *
 * Caller contract.  Triangle k (binding 3) and ellipsoid k (binding 7) of the buffers uploaded after the mark must be the same piece of
 * surface as triangle k and ellipsoid k at the mark; only its position may change.  A changed topology is out of scope.  So is lighting that
 * changes away from the moved object: moved shadows and reflections keep their stale history until max_history ages it out.
 *
 * The mark.  On the device: (a) the feature records of include/pt_denoise.h under the image's camera in the scene as it is at the mark (Rh),
 * W*H*64 B; (b) per triangle of binding 3 its three vertices (floats 0-2, 4-6, 8-10 of the 40-float record) as three float4: 48 B per
 * triangle; (c) per ellipsoid of binding 7 its centre, stretch, rot and r as three float4: 48 B per ellipsoid; and on the host 36 B per
 * triangle and 40 B per ellipsoid of the same values (to find the moved ones), (d) the image's index, its camera record and a count of the
 * non-geometry uploads.  pt_reproject_frame_moved adds the same 48 B per primitive of the current scene, packed once per call.
 *
 * Mapping.  include/pt_reproject.h's, steps 1, 3, 4, 6 and 7 unchanged (step 7 of include/pt_demod.h when albedo_floor > 0); binary32
 * * + - / sqrt in the written order, no fused multiply-add.  dot(a,b) = (a0*b0 + a1*b1) + a2*b2; cross(a,b) = (a1*b2 - a2*b1,
 * a2*b0 - a0*b2, a0*b1 - a1*b0); vectors work per component.  ' marks the values of the mark, except O', M', ss', fl', hr', which stay the image's camera.
 *   2. Hit / miss split and rejections as before.  A hit computes P = O + t*D and, from its hit code type*0x1000000 + id, the point P'
 *      where that surface point was at the mark and the normal N~ it had there:
 *      Triangle k (type 1): rejected unless k is below the triangle count of the mark and of the current binding 3.  A, B, C = its vertices
 *        now, A', B', C' = at the mark.  Unmoved (all nine floats compare equal): P' = P, N~ = N, bit for bit.  Moved:
 *          e1 = B - A, e2 = C - A, w = P - A, e1' = B' - A', e2' = C' - A'
 *          d11 = dot(e1,e1), d12 = dot(e1,e2), d22 = dot(e2,e2), den = d11*d22 - d12*d12; rejected unless den is finite and > 0
 *          beta = (d22*dot(w,e1) - d12*dot(w,e2)) / den, gamma = (d11*dot(w,e2) - d12*dot(w,e1)) / den
 *          P' = (A' + beta*e1') + gamma*e2'
 *          g = cross(e1,e2), g' = cross(e1',e2')
 *          a = (d22*dot(N,e1) - d12*dot(N,e2)) / den, b = (d11*dot(N,e2) - d12*dot(N,e1)) / den, c = dot(N,g) / dot(g,g)
 *          M = (a*e1' + b*e2') + c*g', N~ = M / sqrt(dot(M,M)); rejected if P' or N~ is not finite.
 *        (N's components along e1, e2 and the face normal, put back on the old edges.)  Exact for a rigid motion, up to rounding; for any other
 *        deformation an approximation of the old shading normal that normal_tol absorbs.
 *      Ellipsoid k (type 3): rejected unless k is below both ellipsoid counts.  Unmoved (centre, stretch, rot and r, ten floats, compare
 *        equal): P' = P, N~ = N.  A moved ellipsoid with a rot component != 0 then or now is rejected (the shader's rotated branch goes
 *        through its own sin / cos; a rejection is always safe: the pixel restarts).  Otherwise u = P - c,
 *        k_i = sqrt(stretch_i / stretch'_i) * (r' / r), P' = c' + u*k, N~ = N; rejected if P' is not finite.
 *      Any other type: rejected.
 *      Hit: v = P' - O'.  Miss: v = D, as before.
 *   5. Rh is the mark's; the depth test uses |v| as before, the normal test N~ in place of N, the material test is unchanged.
 * With no primitive moved the result is pt_reproject_frame's (pt_reproject_frame_demod's) bit for bit.  Of the image's camera only camRot,
 * the origin, screenSize, focalLength and screenHratio enter, so that building its frame constants in the new scene changes nothing.
 */
#ifndef PT_MOTION_H
#define PT_MOTION_H
#include "pt_reproject.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Pins the scene the current image was rendered in (see "The mark" above).  Completes all submitted work first.  A second mark replaces the
 * first; the mark is freed with the context.  FRAME and T are not touched.
 * PT_ERR_ARG: null context; the current image has no camera; a scene buffer (any binding but 0, 1, 2, 4) or a texture was uploaded since that
 * camera was recorded; the camera's Parameters do not match the image size.
 * PT_ERR_UNSUPPORTED: the image was rendered with Parameters.DEBUG != 0; a context that holds only part of the image. */
int pt_motion_mark(pt_ctx* ctx);

/* pt_reproject_frame with Rh and the primitives' old positions taken from the mark, by the mapping above.  albedo_floor == 0: step 7 of
 * include/pt_reproject.h; > 0 (and finite): step 7 of include/pt_demod.h with that floor.  Between the mark and the call the geometry
 * bindings 3, 7, 10, 11, 12, 13 and the frame inputs 0, 1, 2, 4 may be uploaded.  On success the current inputs become the image's camera,
 * recorded in the current scene, and the mark is spent.  One-stream and pt_create_multi contexts give identical results.
 * PT_ERR_ARG: what pt_reproject_frame names for its arguments and Parameters; albedo_floor negative, NaN or infinite; no mark; the mark
 * belongs to another image; the image's camera record is no longer the marked one (a render, pt_write_frame, pt_reset_frame or
 * pt_next_image since the mark); binding 14, binding 5 or a texture uploaded since the mark.
 * PT_ERR_UNSUPPORTED: as pt_reproject_frame.  On every error FRAME and T are unchanged. */
int pt_reproject_frame_moved(pt_ctx* ctx, float max_history, float depth_tol, float normal_tol, int flags, float albedo_floor, int64_t* n_kept);

#ifdef __cplusplus
}
#endif
#endif
