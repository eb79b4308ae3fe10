// pt_denoise.hip — the edge-avoiding a-trous filter of include/pt_denoise.h (Dammertz et al. 2010) for gfx950.
//
// Device pointers only: pt_hip.hip owns the buffers, computes the feature records and calls denoiseLaunch on its stream.
//   k_dn_prep    per pixel: the mean FRAME.rgb / FRAME.a (raw rgb when FRAME.a <= 0), the pixel's class (0 invalid, 1 hit, 2 miss)
//                in w, and the guide (t, N), (Kd, -) packed into 32 B so that a tap reads two adjacent float4 of the feature record's four
//   k_dn_pass    one pass of step 2^i: one pixel per lane, a wave = 64 pixels of a row, a block = 4 rows; the 25 taps are served by
//                L2 (every tap row of a wave is 1 KiB of colour + 2 KiB of guide, contiguous)
//   k_dn_finish  (denoised rgb, FRAME.a)
// Not under the bit-exact contract of the render path: __expf, and the summation order is the tap loop's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_image_launch.hpp"

namespace {

constexpr int DN_BX = 64, DN_BY = 4;

__device__ __forceinline__ bool finite3(float a, float b, float c) { return __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c); }

__global__ void __launch_bounds__(256) k_dn_prep(const float4* frame, const float4* feat, int n, float4* col, float4* guide) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 F = frame[i], f0 = feat[4 * (size_t)i], f1 = feat[4 * (size_t)i + 1];
    const float a = F.w;
    const float mx = F.x / a, my = F.y / a, mz = F.z / a;
    const bool valid = a > 0.0f && finite3(mx, my, mz) && __builtin_isfinite(f0.x) && finite3(f0.y, f0.z, f0.w) && finite3(f1.x, f1.y, f1.z);
    const float cls = valid ? (__float_as_int(f1.w) >= 0 ? 1.0f : 2.0f) : 0.0f;
    col[i] = a > 0.0f ? make_float4(mx, my, mz, cls) : make_float4(F.x, F.y, F.z, cls);
    guide[2 * (size_t)i] = f0;
    guide[2 * (size_t)i + 1] = make_float4(f1.x, f1.y, f1.z, 0.0f);
}

// inv = (4^i / sc^2, 1 / sn^2, 1 / sd^2, 1 / sa^2), each clamped to FLT_MAX so that a zero difference never meets an infinity
__global__ void __launch_bounds__(DN_BX * DN_BY) k_dn_pass(const float4* __restrict__ in, const float4* __restrict__ guide, float4* __restrict__ out, int W, int H,
                                                           int step, float4 inv) {
    const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float4 cp = in[p];
    if (cp.w == 0.0f) { out[p] = cp; return; }                    // invalid: passed through, weighs no neighbour
    const bool hit = cp.w == 1.0f;
    float4 gp0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gp1 = gp0;
    if (hit) { gp0 = guide[2 * p]; gp1 = guide[2 * p + 1]; }
    const float invT = 1.0f / gp0.x;
    const float h[5] = {1.0f / 16.0f, 4.0f / 16.0f, 6.0f / 16.0f, 4.0f / 16.0f, 1.0f / 16.0f};
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int yy = y + dy * step;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int xx = x + dx * step;
            if (xx < 0 || xx >= W) continue;
            const size_t q = (size_t)yy * W + xx;
            const float4 cq = in[q];
            if (cq.w != cp.w) continue;                           // invalid, or hit against miss
            const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
            float e = (dr * dr + dg * dg + db * db) * inv.x;
            if (hit) {
                const float4 g0 = guide[2 * q], g1 = guide[2 * q + 1];
                const float nx = gp0.y - g0.y, ny = gp0.z - g0.z, nz = gp0.w - g0.w;
                const float dt = (gp0.x - g0.x) * invT;
                const float ar = gp1.x - g1.x, ag = gp1.y - g1.y, ab = gp1.z - g1.z;
                e += (nx * nx + ny * ny + nz * nz) * inv.y + (dt * dt) * inv.z + (ar * ar + ag * ag + ab * ab) * inv.w;
            }
            const float w = (h[dy + 2] * h[dx + 2]) * __expf(-e);
            sr += w * cq.x; sg += w * cq.y; sb += w * cq.z; sw += w;
        }
    }
    out[p] = make_float4(sr / sw, sg / sw, sb / sw, cp.w);
}

__global__ void __launch_bounds__(256) k_dn_finish(const float4* col, const float4* frame, int n, float4* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 c = col[i];
    out[i] = make_float4(c.x, c.y, c.z, frame[i].w);
}

float clampInv(float v) { return v > 3.402823466e38f ? 3.402823466e38f : v; }

}  // namespace

// pt_image_launch.hpp; sigma already checked by the caller
hipError_t denoiseLaunch(const float4* frame, const float4* feat, int W, int H, int iterations, const float sigma[4], float4* col0, float4* col1,
                         float4* guide, float4* out, hipStream_t s) {
    const int n = W * H;
    const dim3 lin((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(k_dn_prep, lin, dim3(256), 0, s, frame, feat, n, col0, guide);
    float4* src = col0;
    float4* dst = col1;
    const float invN = clampInv(1.0f / (sigma[1] * sigma[1])), invD = clampInv(1.0f / (sigma[2] * sigma[2])), invA = clampInv(1.0f / (sigma[3] * sigma[3]));
    const dim3 grid((unsigned)((W + DN_BX - 1) / DN_BX), (unsigned)((H + DN_BY - 1) / DN_BY));
    for (int i = 0; i < iterations; i++) {
        const float invC = clampInv((float)(1 << (2 * i)) / (sigma[0] * sigma[0]));
        hipLaunchKernelGGL(k_dn_pass, grid, dim3(DN_BX, DN_BY), 0, s, src, guide, dst, W, H, 1 << i, make_float4(invC, invN, invD, invA));
        float4* t = src; src = dst; dst = t;
    }
    hipLaunchKernelGGL(k_dn_finish, lin, dim3(256), 0, s, src, frame, n, out);
    return hipGetLastError();
}
