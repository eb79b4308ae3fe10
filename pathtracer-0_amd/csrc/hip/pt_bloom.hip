// pt_bloom.hip — the glare of include/pt_bloom.h for gfx950: the bright pass fused into the first reduction, the pyramid down and up, and the
// composition over the source image.
//
// Device pointers only: pt_bloom_host.hpp owns the path (the source image, the pyramid and the composed image, the exposure) and calls bloomLaunch on
// its stream; the level table, norm and T are pt_bloom_rule.hpp's.  A pyramid texel is a float4 (rgb, 0): every load and store is one 16-B access.
//   k_bl_down_first  steps 0-2 from the source: D_1 from B with no full-size bright image stored.  Each output's 4 x 4 taps overlap its neighbours',
//                so every source pixel is wanted four times, and its bright pass costs a luminance and an IEEE division (three more under FRAME).
//                A 16 x 16 output block stages its 34 x 34 cleaned, bright-passed source tile in LDS (float4, 18.1 KB), one bright pass per
//                source pixel, and takes its taps from there.  The tile's columns are stored evens first, then odds: the lanes of a row read
//                texels two columns apart, which would put lanes l and l + 8 of a ds_read_b128 group on one bank; split so, they read 16 adjacent
//                16-B slots.  The form in which every lane takes its 16 taps from L2 and bright-passes each was built and measured at 1080p:
//                33.8 against 15.2 us on a rendered C3 frame, 34.8 against 15.8 us on a one-colour image, at 78 / 104 VGPRs against 61
//                (DESIGN.md 2.25); it is not in the file.
//   k_bl_down    step 2 between levels: 16 taps from L2 (a quarter of the pixels of the level above, and a quarter again at each level).
//   k_bl_up      step 3, one level per launch, in place: U_k over D_k (a lane reads and writes its own texel of the level, and four of the coarser one).
//   k_bl_compose the last up, norm and step 4: one 16-B load of the source, four of U_1, one 16-B store per pixel.
// Under the bit-exact contract: binary32 * + - / in the header's order, no contraction (the build's -ffp-contract=off, IEEE divide).
#include <hip/hip_runtime.h>

#include "pt_bloom_rule.hpp"
#include "pt_image_launch.hpp"

namespace {

constexpr int BL_B = 16, BL_T = 2 * BL_B + 2;     // a block of the reductions: 16 x 16 outputs; the source tile of one: 34 x 34
constexpr int BL_UX = 64, BL_UY = 4;              // a block of k_bl_up and k_bl_compose: a wave per row segment

__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ float clean(float v) { return (v != v) ? 0.0f : (v < 0.0f ? 0.0f : (v > 65504.0f ? 65504.0f : v)); }

// steps 0-1 of a source texel: B
template <bool PER_PIXEL>
__device__ __forceinline__ float4 brightPass(const float4 F, float T) {
    const bool emits = F.w > 0.0f;                                 // a count of 0, a negative one or a NaN: no glare
    const float r = emits ? clean(PER_PIXEL ? F.x / F.w : F.x) : 0.0f;
    const float g = emits ? clean(PER_PIXEL ? F.y / F.w : F.y) : 0.0f;
    const float b = emits ? clean(PER_PIXEL ? F.z / F.w : F.z) : 0.0f;
    const float l = lum(r, g, b);
    const float k = l > T ? (l - T) / l : 0.0f;
    return make_float4(r * k, g * k, b * k, 0.0f);
}

// the tent (1, 3, 3, 1) / 8 over four texels, in step 2's order
__device__ __forceinline__ float4 tent(const float4 p0, const float4 p1, const float4 p2, const float4 p3) {
    return make_float4((0.125f * p0.x + 0.375f * p1.x) + (0.375f * p2.x + 0.125f * p3.x),
                       (0.125f * p0.y + 0.375f * p1.y) + (0.375f * p2.y + 0.125f * p3.y),
                       (0.125f * p0.z + 0.375f * p1.z) + (0.375f * p2.z + 0.125f * p3.z), 0.0f);
}

// up(V)(x, y) of step 3 for a texel (x, y) of the finer level; V is Wc x Hc
__device__ __forceinline__ float4 upTap(const float4* __restrict__ V, int Wc, int Hc, int x, int y) {
    const int cx = x >> 1, cy = y >> 1;
    const int nx = clampi(cx + ((x & 1) ? 1 : -1), Wc - 1), ny = clampi(cy + ((y & 1) ? 1 : -1), Hc - 1);
    const float4 a = V[(size_t)cy * Wc + cx], b = V[(size_t)cy * Wc + nx], c = V[(size_t)ny * Wc + cx], d = V[(size_t)ny * Wc + nx];
    return make_float4((0.5625f * a.x + 0.1875f * b.x) + (0.1875f * c.x + 0.0625f * d.x),
                       (0.5625f * a.y + 0.1875f * b.y) + (0.1875f * c.y + 0.0625f * d.y),
                       (0.5625f * a.z + 0.1875f * b.z) + (0.1875f * c.z + 0.0625f * d.z), 0.0f);
}

template <bool PER_PIXEL>
__global__ void __launch_bounds__(BL_B * BL_B) k_bl_down_first(const float4* __restrict__ src, int W, int H, float T, float4* __restrict__ dst, int Wd, int Hd) {
    __shared__ float4 tile[BL_T * BL_T];
    const int x0 = 2 * (int)blockIdx.x * BL_B - 1, y0 = 2 * (int)blockIdx.y * BL_B - 1;
    for (int i = threadIdx.y * BL_B + threadIdx.x; i < BL_T * BL_T; i += BL_B * BL_B) {      // every lane of the block, in range or not
        const int tx = i % BL_T, ty = i / BL_T;
        const float4 F = src[(size_t)clampi(y0 + ty, H - 1) * W + clampi(x0 + tx, W - 1)];
        tile[ty * BL_T + (tx & 1) * (BL_T / 2) + (tx >> 1)] = brightPass<PER_PIXEL>(F, T);
    }
    __syncthreads();
    const int x = blockIdx.x * BL_B + threadIdx.x, y = blockIdx.y * BL_B + threadIdx.y;
    if (x >= Wd || y >= Hd) return;
    // taps 2*lx + (0, 1, 2, 3): the even columns lx, lx + 1 and the odd ones lx, lx + 1
    const float4* t = tile + 2 * threadIdx.y * BL_T + threadIdx.x;
    float4 row[4];
#pragma unroll
    for (int j = 0; j < 4; j++) row[j] = tent(t[j * BL_T], t[j * BL_T + BL_T / 2], t[j * BL_T + 1], t[j * BL_T + BL_T / 2 + 1]);
    dst[(size_t)y * Wd + x] = tent(row[0], row[1], row[2], row[3]);
}

__global__ void __launch_bounds__(BL_B * BL_B) k_bl_down(const float4* __restrict__ src, int W, int H, float4* __restrict__ dst, int Wd, int Hd) {
    const int x = blockIdx.x * BL_B + threadIdx.x, y = blockIdx.y * BL_B + threadIdx.y;
    if (x >= Wd || y >= Hd) return;
    float4 row[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float4* r = src + (size_t)clampi(2 * y - 1 + j, H - 1) * W;
        row[j] = tent(r[clampi(2 * x - 1, W - 1)], r[2 * x], r[clampi(2 * x + 1, W - 1)], r[clampi(2 * x + 2, W - 1)]);
    }
    dst[(size_t)y * Wd + x] = tent(row[0], row[1], row[2], row[3]);
}

// fine holds D_k and leaves as U_k
__global__ void __launch_bounds__(BL_UX * BL_UY) k_bl_up(const float4* __restrict__ coarse, int Wc, int Hc, float4* __restrict__ fine, int W, int H, float spread) {
    const int x = blockIdx.x * BL_UX + threadIdx.x, y = blockIdx.y * BL_UY + threadIdx.y;
    if (x >= W || y >= H) return;
    const float4 u = upTap(coarse, Wc, Hc, x, y);
    const size_t i = (size_t)y * W + x;
    const float4 d = fine[i];
    fine[i] = make_float4(d.x + spread * u.x, d.y + spread * u.y, d.z + spread * u.z, 0.0f);
}

template <bool PER_PIXEL>
__global__ void __launch_bounds__(BL_UX * BL_UY) k_bl_compose(const float4* __restrict__ src, int W, int H, const float4* __restrict__ U1, int Wc, int Hc,
                                                             float norm, float intensity, float4* __restrict__ out) {
    const int x = blockIdx.x * BL_UX + threadIdx.x, y = blockIdx.y * BL_UY + threadIdx.y;
    if (x >= W || y >= H) return;
    const float4 u = upTap(U1, Wc, Hc, x, y);
    const size_t i = (size_t)y * W + x;
    const float4 F = src[i];
    const float r = PER_PIXEL ? F.x / F.w : F.x, g = PER_PIXEL ? F.y / F.w : F.y, b = PER_PIXEL ? F.z / F.w : F.z;
    out[i] = make_float4(r + intensity * (u.x * norm), g + intensity * (u.y * norm), b + intensity * (u.z * norm), F.w);
}

dim3 gridOf(int W, int H, int bx, int by) { return dim3((unsigned)((W + bx - 1) / bx), (unsigned)((H + by - 1) / by)); }

}  // namespace

hipError_t bloomLaunch(const BloomJob& j, hipStream_t s) {
    if (!j.image || !j.pyramid || !j.out || j.out == j.image || j.W <= 0 || j.H <= 0 || j.levels < 1 || j.levels > PT_BLOOM_MAX_LEVELS) return hipErrorInvalidValue;
    if ((j.H + BL_UY - 1) / BL_UY > 65535) return hipErrorInvalidValue;      // the grid's y extent
    const ptp::BloomPyramid p = ptp::bloomPyramid(j.W, j.H, j.levels);
    const ptp::BloomLevel* v = p.level;
    const dim3 red(BL_B, BL_B), wide(BL_UX, BL_UY);
    if (j.perPixel) hipLaunchKernelGGL(k_bl_down_first<true>, gridOf(v[1].W, v[1].H, BL_B, BL_B), red, 0, s, j.image, j.W, j.H, j.T, j.pyramid + v[1].offset, v[1].W, v[1].H);
    else hipLaunchKernelGGL(k_bl_down_first<false>, gridOf(v[1].W, v[1].H, BL_B, BL_B), red, 0, s, j.image, j.W, j.H, j.T, j.pyramid + v[1].offset, v[1].W, v[1].H);
    for (int k = 1; k < j.levels; k++)
        hipLaunchKernelGGL(k_bl_down, gridOf(v[k + 1].W, v[k + 1].H, BL_B, BL_B), red, 0, s, (const float4*)(j.pyramid + v[k].offset), v[k].W, v[k].H,
                           j.pyramid + v[k + 1].offset, v[k + 1].W, v[k + 1].H);
    for (int k = j.levels - 1; k >= 1; k--)
        hipLaunchKernelGGL(k_bl_up, gridOf(v[k].W, v[k].H, BL_UX, BL_UY), wide, 0, s, (const float4*)(j.pyramid + v[k + 1].offset), v[k + 1].W, v[k + 1].H,
                           j.pyramid + v[k].offset, v[k].W, v[k].H, j.spread);
    if (j.perPixel) hipLaunchKernelGGL(k_bl_compose<true>, gridOf(j.W, j.H, BL_UX, BL_UY), wide, 0, s, j.image, j.W, j.H, (const float4*)(j.pyramid + v[1].offset), v[1].W, v[1].H,
                                       j.norm, j.intensity, j.out);
    else hipLaunchKernelGGL(k_bl_compose<false>, gridOf(j.W, j.H, BL_UX, BL_UY), wide, 0, s, j.image, j.W, j.H, (const float4*)(j.pyramid + v[1].offset), v[1].W, v[1].H,
                            j.norm, j.intensity, j.out);
    return hipGetLastError();
}
