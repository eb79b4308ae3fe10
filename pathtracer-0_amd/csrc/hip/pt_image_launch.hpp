// pt_image_launch.hpp — the launch interface of the image-space passes: pt_denoise.hip, pt_guided.hip and pt_reproject.hip define these functions,
// pt_image.hpp (the host half, inside pt_hip.hip) calls them.  Device pointers only; everything is enqueued on the stream given and the first
// launch error is returned.  A job is a plain struct: the caller checks the values, the launch reads them.
#pragma once
#include <hip/hip_runtime.h>

namespace ptd { struct FrameConst; }

// ---- the a-trous filter of include/pt_denoise.h (pt_denoise.hip)
// frame, feat: W*H float4 / W*H*4 float4 (read only); col0, col1: W*H float4 ping-pong; guide: 2*W*H float4; out: W*H float4.
// sigma = (colour, normal, depth, albedo)
hipError_t denoiseLaunch(const float4* frame, const float4* feat, int W, int H, int iterations, const float sigma[4], float4* col0, float4* col1,
                         float4* guide, float4* out, hipStream_t s);

// ---- the variance-guided filter of include/pt_guided.h, its selection (pt_steer.h), demodulation (pt_demod.h) and prefill (pt_fill.h) (pt_guided.hip)
struct GuidedJob {
    // the inputs.  frame, stats: W*H float4 (FRAME and T in pixel order), feat: W*H*4 float4, all read only
    const float4* frame = nullptr; const float4* feat = nullptr; const float4* stats = nullptr;
    int W = 0, H = 0, iterations = 0;
    float sigma[4] = {1.0f, 1.0f, 1.0f, 1.0f};                    // (luminance, normal, depth, albedo)
    int minFrames = 2;
    float floorA = 0.0f;                                          // 0: the plain kernels; > 0: the demodulated ones, with that albedo_floor
    float4* col0 = nullptr; float4* col1 = nullptr;               // scratch: W*H float4 ping-pong
    float4* guide = nullptr;                                      // scratch: 2*W*H float4
    // the optional prefill: FRAME' into fill[W*H] and the holes filled into *fillCount (zeroed first); the filter then runs on FRAME' and takes
    // its output's alpha from the real FRAME
    float4* fill = nullptr; unsigned* fillCount = nullptr;
    // the output, one of: the filtered image out[W*H] (null with `fill`: the prefill alone); or mask[W*H] and *count (zeroed first) of pt_steer.h's rule
    float4* out = nullptr;
    unsigned char* mask = nullptr; unsigned* count = nullptr;
    int maxFrames = 0; float relErr = 0.0f, absErr = 0.0f;
    float overlay[3] = {0.0f, 0.0f, 0.0f};                        // (mouse x, mouse y, resolution) of the overlay test
};
// prep, the variance (the filter: when iterations > 0; the selection: always), `iterations` passes, then finish or select
hipError_t guidedLaunch(const GuidedJob& j, hipStream_t s);

// ---- the reprojection of include/pt_reproject.h, pt_demod.h, pt_motion.h, pt_reproject_through.h, pt_reproject_bilinear.h and pt_motion_bilinear.h (pt_reproject.hip).  The three structs are kernel arguments as they stand.
struct ReprojCam {
    float On[3];                        // the current ORIGIN (the origin of Rn's rays)
    float mouseX, mouseY, resolution;   // the current mouse overlay
};
struct ReprojRule { float maxHistory, depthTol, normalTol; int allMaterials; };
// Geometry: 3 float4 per primitive, then (the mark) and now (packed by the host once per call).  Triangle: (A, flag), (B, 0), (C, 0); ellipsoid:
// (c, r), (stretch, flag), (rot, 0).  flag (int bits, "now" only): 0 unmoved, 1 moved, 2 a moved ellipsoid with a rotation (rejected).
struct ReprojMotion {
    const float4* triNow; const float4* triThen; int nTriNow, nTriThen;
    const float4* elNow; const float4* elThen; int nElNow, nElThen;
};
struct ReprojectJob {
    // rn, rh: W*H*4 float4 feature records under the current inputs / the image's camera; frame, stats: the image's FRAME and T (stats may be
    // null), W*H float4 in pixel order; hist: the frame constants k_frame_setup built from the image's camera; matVD: nMat bytes, 1 = view-dependent
    const float4* rn = nullptr; const float4* rh = nullptr; const float4* frame = nullptr; const float4* stats = nullptr;
    const ptd::FrameConst* hist = nullptr; const unsigned char* matVD = nullptr;
    int nMat = 0, W = 0, H = 0;
    ReprojCam cam{};
    ReprojRule rule{};
    float floorA = 0.0f;                                          // 0: pt_reproject.h's step 7; > 0: pt_demod.h's, with that albedo_floor
    const ReprojMotion* motion = nullptr;                         // given: pt_motion.h's mapping, rh and the "then" geometry from the mark
    bool bilinear = false; float snap = 0.0f;                     // include/pt_reproject_bilinear.h's taps (no sn; with motion: include/pt_motion_bilinear.h's); kept[1]: the blended pixels
    // include/pt_reproject_through.h, when sn is given (no motion, floorA 0): sn, yn / sh, yh: the seen-through records (W*H*4 float4) and their last
    // segments (W*H*2 float4) under the current inputs / the image's camera; pack: scratch, W*H*2 float4; radius: 0 .. 4 (checked by the caller)
    const float4* sn = nullptr; const float4* yn = nullptr; const float4* sh = nullptr; const float4* yh = nullptr;
    float4* pack = nullptr; float pointTol = 0.0f; int radius = 0;
    // outFrame (and outStats when stats is given): W*H float4; *kept (zeroed first): the pixels kept; with sn, kept[1]: those among them with a chain
    float4* outFrame = nullptr; float4* outStats = nullptr; unsigned* kept = nullptr;
};
hipError_t reprojectLaunch(const ReprojectJob& j, hipStream_t s);

// ---- the history validation of include/pt_validate.h (pt_reproject.hip)
struct ValidateJob {
    // feat: W*H*4 float4 feature records under the current inputs; frame, stats: FRAME and T now (N, U); heldFrame, heldStats: the held ones (H, V);
    // all W*H float4 in pixel order, read only
    const float4* feat = nullptr; const float4* frame = nullptr; const float4* stats = nullptr;
    const float4* heldFrame = nullptr; const float4* heldStats = nullptr;
    int W = 0, H = 0, radius = 0;                                 // radius: 1 .. 4 (checked by the caller)
    float zLo = 0.0f, zHi = 0.0f, normalTol = 0.0f;
    float overlay[3] = {0.0f, 0.0f, 0.0f};                        // (mouse x, mouse y, resolution) of the overlay test
    // outFrame, outStats: W*H float4; kappa: W*H floats, or null; *reduced (zeroed first): the pixels with H.a > 0 and kappa < 1
    float4* outFrame = nullptr; float4* outStats = nullptr; float* kappa = nullptr; unsigned* reduced = nullptr;
};
hipError_t validateLaunch(const ValidateJob& j, hipStream_t s);

// ---- the outlier rejection of include/pt_despeckle.h (pt_despeckle.hip)
struct DespeckleJob {
    // feat: W*H*4 float4 feature records under the current inputs; frame, stats: FRAME and T in pixel order (stats may be null: step 5 is off then),
    // W*H float4, read only
    const float4* feat = nullptr; const float4* frame = nullptr; const float4* stats = nullptr;
    int W = 0, H = 0, radius = 0, minTaps = 0;                    // radius: 1 .. 3 (checked by the caller)
    float sigmas = 0.0f, ownZ = 0.0f, normalTol = 0.0f, minLum = 0.0f;
    float overlay[3] = {0.0f, 0.0f, 0.0f};                        // (mouse x, mouse y, resolution) of the overlay test
    bool mean = false;                                            // outFrame takes (the rule applied to the mean, FRAME.a) in place of FRAME'
    // outFrame: W*H float4; outStats: T', W*H float4, or null (needs stats); scale: W*H floats, or null; *clamped (zeroed first): the pixels clamped
    float4* outFrame = nullptr; float4* outStats = nullptr; float* scale = nullptr; unsigned* clamped = nullptr;
};
hipError_t despeckleLaunch(const DespeckleJob& j, hipStream_t s);

// ---- the display image of include/pt_tonemap.h (pt_tonemap.hip)
struct TonemapJob {
    // image: W*H float4 in pixel order, read only.  perPixel: it is FRAME (rgb a running sum, divided by the pixel's own count a); else rgb is a
    // mean already and a carries FRAME.a
    const float4* image = nullptr; bool perPixel = false;
    int W = 0, H = 0;
    // either or both of: hist[PT_TONEMAP_BINS] (zeroed first): steps 1-2;  bytes[W*H*3], top row first: steps 4-5 under the values below
    unsigned* hist = nullptr;
    unsigned char* bytes = nullptr;
    float exposure = 1.0f, white = 1.0f;
    int curve = 0, transfer = 0;                                  // 0 .. 2 and 0 .. 1 (checked by the caller)
};
hipError_t tonemapLaunch(const TonemapJob& j, hipStream_t s);

// ---- the glare of include/pt_bloom.h (pt_bloom.hip)
struct BloomJob {
    // image: W*H float4 in pixel order, read only.  perPixel: it is FRAME (rgb a running sum, divided by the pixel's own count a); else rgb is a
    // mean already and a carries FRAME.a
    const float4* image = nullptr; bool perPixel = false;
    int W = 0, H = 0, levels = 0;                                 // levels: 1 .. PT_BLOOM_MAX_LEVELS (checked by the caller)
    float T = 0.0f, spread = 1.0f, norm = 1.0f, intensity = 0.0f; // T = threshold / exposure and norm: pt_bloom_rule.hpp's
    // pyramid: ptp::bloomPyramid(W, H, levels).texels float4 of scratch;  out: W*H float4, the composed image (not `image`)
    float4* pyramid = nullptr; float4* out = nullptr;
};
hipError_t bloomLaunch(const BloomJob& j, hipStream_t s);
