// pt_tonemap.hip — the display image of include/pt_tonemap.h for gfx950: the luminance histogram and the exposed, tone-mapped, encoded bytes.
//
// Device pointers only: pt_tonemap_host.hpp owns the path (the image, the scratch, the exposure between the two kernels) and calls tonemapLaunch
// on its stream.
//   k_tm_histogram  grid-stride over the pixels, one 16-B load per lane and step; steps 1-2 of the rule; a 512-bin histogram per block in LDS,
//                the block's nonzero bins flushed with one global atomic each.  Integer counts: no order of the atomics shows in the result.
//                Every metered lane does its own LDS add.  A flat region — a wall, the sky, a black background — puts a whole wave into one
//                bin; merging a wave's equal bins first (a ballot over the leading lane's bin, one add of the popcount) was built and
//                measured at 1080p: 14.7 against 15.3 us on a one-colour image, 19.7 against 18.0 us on a rendered C3 frame.  The LDS
//                unit takes 64 adds to one address nearly as fast as 64 adds to many, so the merge is not in the kernel.
//   k_tm_apply   one lane per pixel: steps 4-5.  T, the sRGB threshold table, is staged in LDS (1 KB) and searched in 8 steps per channel; the
//                vertical flip is done on the store, three byte stores per pixel as k_display's.
// Under the bit-exact contract: binary32 * + / in the header's order, no contraction (the build's -ffp-contract=off, IEEE divide).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_image_launch.hpp"
#include "pt_tonemap_rule.hpp"

namespace {

constexpr int TM_BLOCK = 256, TM_BINS = PT_TONEMAP_BINS;
constexpr unsigned TM_HIST_BLOCKS = 512;      // few on purpose: every used bin takes one serialised global add per block (2048: 44 us, 8192: 143 us at 1080p)

__constant__ float tmSrgbThresholds[256] = {PT_TONEMAP_SRGB_THRESHOLDS};

__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// PER_PIXEL: the image is FRAME (rgb a running sum, a its count); else rgb is a mean already
template <bool PER_PIXEL>
__global__ void __launch_bounds__(TM_BLOCK) k_tm_histogram(const float4* __restrict__ image, size_t n, unsigned* __restrict__ hist) {
    __shared__ unsigned bins[TM_BINS];
    for (int t = threadIdx.x; t < TM_BINS; t += TM_BLOCK) bins[t] = 0;
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * TM_BLOCK;
    for (size_t i = (size_t)blockIdx.x * TM_BLOCK + threadIdx.x; i < n; i += stride) {
        const float4 F = image[i];
        const float l = PER_PIXEL ? lum(F.x / F.w, F.y / F.w, F.z / F.w) : lum(F.x, F.y, F.z);
        const bool metered = F.w > 0.0f && __builtin_isfinite(l) && l > 0.0f;
        int b = (int)(__float_as_uint(l) >> 19) - 1776;
        b = b < 0 ? 0 : (b > TM_BINS - 1 ? TM_BINS - 1 : b);
        if (metered) atomicAdd(&bins[b], 1u);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < TM_BINS; t += TM_BLOCK) {
        const unsigned v = bins[t];
        if (v) atomicAdd(&hist[t], v);
    }
}

struct TonemapApply { float exposure, white2; int curve, transfer; };

template <bool PER_PIXEL>
__global__ void __launch_bounds__(TM_BLOCK) k_tm_apply(const float4* __restrict__ image, int W, int H, TonemapApply a, unsigned char* __restrict__ out) {
    __shared__ float T[256];
    T[threadIdx.x] = tmSrgbThresholds[threadIdx.x];
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * TM_BLOCK + threadIdx.x;
    if (i >= (size_t)W * H) return;
    const int x = (int)(i % (size_t)W), y = (int)(i / (size_t)W);
    const float4 F = image[i];
    const float v[3] = {PER_PIXEL ? F.x / F.w : F.x, PER_PIXEL ? F.y / F.w : F.y, PER_PIXEL ? F.z / F.w : F.z};
    const bool shown = F.w > 0.0f;                                 // a count of 0, a negative one or a NaN: black
    int q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float xk = v[k] * a.exposure;
        xk = (xk != xk) ? 0.0f : (xk < 0.0f ? 0.0f : (xk > 65504.0f ? 65504.0f : xk));
        float t = xk;
        if (a.curve == 1) t = (xk * (1.0f + xk / a.white2)) / (1.0f + xk);
        else if (a.curve == 2) t = (xk * (2.51f * xk + 0.03f)) / (xk * (2.43f * xk + 0.59f) + 0.14f);
        t = (t != t) ? 0.0f : (t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t));
        if (!shown) t = 0.0f;
        if (a.transfer == 0) q[k] = (int)__builtin_floorf(t * 255.0f + 0.5f);
        else {
            int lo = 0;                                            // the largest k with T[k] <= t: T[0] = 0 <= t always
#pragma unroll
            for (int step = 128; step >= 1; step >>= 1) lo += T[lo + step] <= t ? step : 0;
            q[k] = lo;
        }
    }
    unsigned char* o = out + 3 * ((size_t)(H - 1 - y) * W + x);
    o[0] = (unsigned char)q[0]; o[1] = (unsigned char)q[1]; o[2] = (unsigned char)q[2];
}

}  // namespace

hipError_t tonemapLaunch(const TonemapJob& j, hipStream_t s) {
    if (!j.image || j.W <= 0 || j.H <= 0) return hipErrorInvalidValue;
    const size_t n = (size_t)j.W * j.H;
    const size_t blocks = (n + TM_BLOCK - 1) / TM_BLOCK;
    if (j.hist) {
        hipError_t e = hipMemsetAsync(j.hist, 0, TM_BINS * sizeof(unsigned), s);
        if (e != hipSuccess) return e;
        const dim3 grid((unsigned)(blocks < TM_HIST_BLOCKS ? blocks : TM_HIST_BLOCKS)), block(TM_BLOCK);
        if (j.perPixel) hipLaunchKernelGGL(k_tm_histogram<true>, grid, block, 0, s, j.image, n, j.hist);
        else hipLaunchKernelGGL(k_tm_histogram<false>, grid, block, 0, s, j.image, n, j.hist);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (j.bytes) {
        if (j.curve < 0 || j.curve > 2 || j.transfer < 0 || j.transfer > 1) return hipErrorInvalidValue;
        const TonemapApply a{j.exposure, j.white * j.white, j.curve, j.transfer};
        const dim3 grid((unsigned)blocks), block(TM_BLOCK);
        if (j.perPixel) hipLaunchKernelGGL(k_tm_apply<true>, grid, block, 0, s, j.image, j.W, j.H, a, j.bytes);
        else hipLaunchKernelGGL(k_tm_apply<false>, grid, block, 0, s, j.image, j.W, j.H, a, j.bytes);
        return hipGetLastError();
    }
    return hipSuccess;
}
