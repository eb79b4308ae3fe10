// pt_despeckle.hip — the outlier rejection of include/pt_despeckle.h for gfx950.
//
// Device pointers only: pt_hip.hip owns the buffers and computes the feature records, pt_despeckle_host.hpp calls despeckleLaunch on its stream.
//   k_despeckle<R>  one lane per pixel, a wave = 64 pixels of a row, a block = 16 rows (k_history_merge's blocks).  The block's tile with its halo of R
//                pixels is staged in LDS once, as five planes of floats: the luminance of the mean, the normal, and one class / material word.  A tile
//                pixel is loaded from global memory once per block (16 B of FRAME, 16 B of F0, the two words of the record) and its three divisions
//                and its luminance are done there, once; a tap then costs five LDS reads of consecutive words per wave and no global load.
//                Steps 1-6, then the clamped count: a ballot popcount per wave, summed in LDS, one global atomic per block.
// No hand-off between blocks: the kernel writes scratch images, never the image it reads, and neighbouring blocks read each other's halo from
// global memory.
// Under the bit-exact contract: binary32 * + / sqrt in the header's order, no contraction (the build's -ffp-contract=off, IEEE divide and sqrt).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_device.hpp"
#include "pt_image_launch.hpp"

using namespace ptd;

namespace {

constexpr int DS_BX = 64, DS_BY = 16;

__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ float dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
// max(x, 0) of include/pt_guided.h: a NaN is no estimate
__device__ __forceinline__ float clampVar(float x) { return x >= 0.0f ? x : (x < 0.0f ? 0.0f : __builtin_inff()); }

// The word plane: the material word of a measured hit, -1 for a measured miss — k_feature_record gives a hit the index of its material, never a
// negative one — and -2 for a pixel outside the image or not measured.  No centre that reaches step 2 has -2, so "in the image, measured, p's
// class and, for a hit, p's material" is one integer compare.  The luminance of a -2 pixel is stored as +0, and every tap is a selected add: a
// tap that does not count adds +0.  S and Q start at +0, and x + (+0) == x bit for bit for every x a sum can hold: a sum that started at +0 is
// never -0 (+0 + -0 = +0 under round-to-nearest), and an inf or a NaN stays what it is.  So the sums equal, bit for bit, those of a model that
// skips the taps that do not count — the header's sums.  The centre is excluded by the same select, never by subtracting it back out (which
// would round differently).
struct DespeckleRule { float sigmas; int minTaps; float ownZ, normalTol, minLum, mouseX, mouseY, resolution; int mean; };
template <int R>
__global__ void __launch_bounds__(DS_BX * DS_BY) k_despeckle(const float4* __restrict__ rec, const float4* __restrict__ frame, const float4* __restrict__ stats,
                                                            int W, int H, DespeckleRule r, float4* __restrict__ outFrame, float4* __restrict__ outStats,
                                                            float* __restrict__ scaleOut, unsigned* __restrict__ clamped) {
    constexpr int TW = DS_BX + 2 * R, TH = DS_BY + 2 * R, TN = TW * TH;
    enum { LUM, NX, NY, NZ, WORD, PLANES };
    __shared__ float tile[PLANES][TN];
    __shared__ unsigned blockClamped;
    const int tid = threadIdx.y * DS_BX + threadIdx.x;
    if (tid == 0) blockClamped = 0;
    const int x0 = blockIdx.x * DS_BX - R, y0 = blockIdx.y * DS_BY - R;
    for (int i = tid; i < TN; i += DS_BX * DS_BY) {
        const int gx = x0 + i % TW, gy = y0 + i / TW;
        float4 f0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float l = 0.0f;
        int word = -2;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gy * W + gx;
            const float4 F = frame[g];
            f0 = rec[4 * g];
            const float* w = reinterpret_cast<const float*>(rec + 4 * g);
            const float lq = lum(F.x / F.w, F.y / F.w, F.z / F.w);
            if (F.w > 0.0f && __builtin_isfinite(lq)) {
                l = lq;
                word = __float_as_int(w[7]) != -1 ? __float_as_int(w[11]) : -1;
            }
        }
        tile[LUM][i] = l; tile[NX][i] = f0.y; tile[NY][i] = f0.z; tile[NZ][i] = f0.w; tile[WORD][i] = __int_as_float(word);
    }
    __syncthreads();
    const int x = blockIdx.x * DS_BX + threadIdx.x, y = blockIdx.y * DS_BY + threadIdx.y;
    const bool in = x < W && y < H;
    bool clamp = false;
    if (in) {
        const size_t p = (size_t)y * W + x;
        const int c = (threadIdx.y + R) * TW + threadIdx.x + R;
        const float lp = tile[LUM][c];
        const int word = __float_as_int(tile[WORD][c]);
        float s = 1.0f;
        FrameConst fc;
        fc.mouse[0] = r.mouseX; fc.mouse[1] = r.mouseY; fc.resolution = r.resolution;
        if (word != -2 && !inMouseOverlay(fc, x, y)) {                                     // 1
            const float Nx = tile[NX][c], Ny = tile[NY][c], Nz = tile[NZ][c];
            int K = 0;
            float S = 0.0f, Q = 0.0f;
#pragma unroll 1
            for (int dy = -R; dy <= R; dy++) {                                             // 2: a row of taps at a time in registers
#pragma unroll
                for (int dx = -R; dx <= R; dx++) {
                    const int q = c + dy * TW + dx;
                    const float lq = tile[LUM][q];
                    const bool tap = (dx != 0 || dy != 0) && __float_as_int(tile[WORD][q]) == word &&
                                     (word == -1 || dot3(Nx, Ny, Nz, tile[NX][q], tile[NY][q], tile[NZ][q]) >= r.normalTol);
                    K += tap ? 1 : 0;
                    S = S + (tap ? lq : 0.0f);
                    Q = Q + (tap ? lq * lq : 0.0f);
                }
            }
            if (K >= r.minTaps) {                                                          // 3
                const float Kf = (float)K, mu = S / Kf;                                    // 4
                const float s2 = clampVar((Q - S * mu) / (Kf - 1.0f));
                float hi = mu + r.sigmas * sqrtf(s2);
                if (hi < r.minLum) hi = r.minLum;
                if (lp > hi) {
                    bool keep = false;
                    if (stats && __builtin_isfinite(r.ownZ)) {                             // 5: T[p] is read by the lanes that got here
                        const float4 T = stats[p];
                        if (T.z >= 2.0f) {
                            const float m = T.x / T.z, s2p = clampVar((T.y - T.x * m) / (T.z - 1.0f));
                            const float v = s2p / frame[p].w, d = lp - mu;
                            keep = d * d > (r.ownZ * r.ownZ) * v;
                        }
                    }
                    if (!keep) { clamp = true; s = hi / lp; }                              // 6
                }
            }
        }
        const float4 F = frame[p];
        float4 o = F;
        if (r.mean) o = make_float4(F.x / F.w, F.y / F.w, F.z / F.w, F.w);
        if (clamp) { o.x = o.x * s; o.y = o.y * s; o.z = o.z * s; }
        outFrame[p] = o;
        if (outStats) {
            float4 T = stats[p];
            if (clamp) T = make_float4(T.x * s, T.y * (s * s), T.z, 0.0f);
            outStats[p] = T;
        }
        if (scaleOut) scaleOut[p] = s;
    }
    const unsigned long long m = __ballot(clamp);                                          // every lane of the block, in range or not
    if (threadIdx.x == 0 && m) atomicAdd(&blockClamped, (unsigned)__popcll(m));
    __syncthreads();
    if (tid == 0 && blockClamped) atomicAdd(clamped, blockClamped);
}

}  // namespace

hipError_t despeckleLaunch(const DespeckleJob& j, hipStream_t s) {
    if (j.outStats && !j.stats) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(j.clamped, 0, 4, s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((j.W + DS_BX - 1) / DS_BX), (unsigned)((j.H + DS_BY - 1) / DS_BY)), block(DS_BX, DS_BY);
    const DespeckleRule r{j.sigmas, j.minTaps, j.ownZ, j.normalTol, j.minLum, j.overlay[0], j.overlay[1], j.overlay[2], j.mean ? 1 : 0};
#define DL_ARGS j.feat, j.frame, j.stats, j.W, j.H, r, j.outFrame, j.outStats, j.scale, j.clamped
    if (j.radius == 1) hipLaunchKernelGGL(k_despeckle<1>, grid, block, 0, s, DL_ARGS);
    else if (j.radius == 2) hipLaunchKernelGGL(k_despeckle<2>, grid, block, 0, s, DL_ARGS);
    else if (j.radius == 3) hipLaunchKernelGGL(k_despeckle<3>, grid, block, 0, s, DL_ARGS);
    else return hipErrorInvalidValue;
#undef DL_ARGS
    return hipGetLastError();
}
