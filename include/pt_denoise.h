/* include/pt_denoise.h — first-hit feature buffers and an edge-aware denoised image on top of include/pt_api.h (libpt_hip.so).
 *
 * No reference counterpart beyond its mouse overlay (frag.glsl:888-893), which shows the first-hit normal of one pixel.  Nothing here
 * changes FRAME, the render path or any other entry point: both surfaces are read-only views of the context's scene and image.
 *
 * Feature record.  PT_FEATURE_FLOATS floats per pixel, 4 float4, in FRAME's pixel order (index y*W + x, as pt_read_frame writes it).
 * Every pixel traces ONE ray: main()'s camera ray (frag.glsl:894-908) with the lens offset zero — the lens-centre ray toward the same
 * focal point (auto-focus and the x mirror included), under the exact numeric contract whatever pt_set_option 16 says.  With
 * BLUR = 0 it is, bit for bit, the primary ray of every sample of the pixel.  The values are the shader's own, quirks included:
 *   F0 = (t, N.x, N.y, N.z)   t = rayScene's distance (-1 on a miss, :651); N = the normal trace() shades with (triangle normal
 *                             selection, ellipsoid normal, map_norm texel), BEFORE the face-forward flip (:830); a triangle without
 *                             vertex normals gives NaN, which stays NaN
 *   F1 = (Kd.r, Kd.g, Kd.b, hit)   Kd after mapMtl (:826); hit = type * 0x1000000 + id as int32 bits (type 1 triangle, 3 ellipsoid), -1 on a miss
 *   F2 = (D.x, D.y, D.z, material) D = the normalised ray direction (the origin is ORIGIN); material index as int32 bits, -1 on a miss
 *   F3 = (u, v, 0, 0)              hit.uvSample: (-1, -1) for a triangle without vt, an ellipsoid inherits the uv of the closest triangle
 *                                  found before it (vec2(0) when there was none)
 * On a miss N, Kd and uv are 0.  A hit is what trace() calls one: a primitive was found and t < 1e25.
 *
 * Denoiser: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010).  c_p = FRAME.rgb / FRAME.a; K = iterations passes,
 * i = 0 .. K-1, the input of pass i being the output of pass i-1.  Pass i has step s = 2^i and the 5x5 B3 taps h = [1,4,6,4,1]/16 at
 * q = p + s*(dx, dy), dx, dy in -2 .. 2:
 *   out_p = sum h(dx) h(dy) w c_q / sum h(dx) h(dy) w
 *   w = exp(-( |c_p - c_q|^2 / (sc^2 * 4^-i) + |N_p - N_q|^2 / sn^2 + ((t_p - t_q) / t_p)^2 / sd^2 + |Kd_p - Kd_q|^2 / sa^2 ))
 * Taps outside the image are skipped.  A hit pixel and a miss pixel never weigh each other; between two miss pixels only the colour
 * term counts.  A pixel is INVALID when FRAME.a <= 0 (never rendered, e.g. the mouse overlay), or its mean is not finite, or one of
 * its t, N, Kd is not finite: it contributes to no neighbour and is passed through unchanged (its mean, or its raw rgb when
 * FRAME.a <= 0).  iterations 0 is the identity.  A sigma of +inf switches its term off.
 * The filter is NOT under the bit-exact contract of the render path: the device uses the hardware exponential (__expf) and its own
 * summation order; a float32 model of the text above agrees to about 1e-4 relative.
 */
#ifndef PT_DENOISE_H
#define PT_DENOISE_H
#include "pt_api.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PT_FEATURE_FLOATS 16

/* Fills out[W*H*16] with the feature records above.  The records are kept on the device and recomputed when pt_set_buffer or
 * pt_set_texture was called since the last computation, otherwise reused.  Synchronous; work in flight is completed first, and
 * later renders are bit-identical to renders without this call.  Works on every context (the scene is replicated; multi-stream
 * and multi-GPU contexts compute the whole image on their first stream's device).
 * PT_ERR_ARG: null context or out, Parameters not set or not matching the image size. */
int pt_read_features(pt_ctx* ctx, float* out);
/* Denoises the current image's per-pixel mean FRAME.rgb / FRAME.a into rgba_out[W*H*4] (rgb = denoised mean, a = FRAME.a), FRAME
 * order.  FRAME itself is not modified.  Computes the feature records first if they are stale (see pt_read_features).
 * PT_ERR_ARG: a null pointer, iterations outside 0 .. 8, a sigma that is NaN or <= 0.
 * PT_ERR_UNSUPPORTED: a context that holds only part of the image (pt_create with shard_count > 1, a pt_create_multi_part group). */
int pt_denoise(pt_ctx* ctx, int iterations, float sigma_color, float sigma_normal, float sigma_depth, float sigma_albedo, float* rgba_out);
/* The same image converted to 8-bit exactly as pt_read_display converts a mean (clamp, round, java_bytes, vertical flip): rgb_out[W*H*3].
 * Errors as pt_denoise. */
int pt_read_display_denoised(pt_ctx* ctx, int iterations, float sigma_color, float sigma_normal, float sigma_depth, float sigma_albedo,
                             int java_bytes, uint8_t* rgb_out);

#ifdef __cplusplus
}
#endif
#endif
