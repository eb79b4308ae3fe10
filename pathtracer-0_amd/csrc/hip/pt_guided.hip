// pt_guided.hip — the variance-guided filter of include/pt_guided.h (the spatial half of Schied et al. 2017) for gfx950.
//
// Device pointers only: pt_hip.hip owns the buffers (the a-trous filter's scratch, shared), computes the feature records, brings T into pixel
// order and calls guidedLaunch on its stream.
//   k_gd_prep    per pixel: the mean FRAME.rgb / FRAME.a (raw rgb when FRAME.a <= 0) and the guide (t, N), (Kd, class) packed into 32 B, the
//                pixel's class (0 invalid, 1 hit, 2 miss) in the second record's w
//   k_gd_var     per pixel: the variance of the mean v = s2 / FRAME.a into the colour record's w; s2 from the pixel's own moments, or pooled
//                over its 7x7 window (same class, same material) when it has fewer than min_frames
//   k_gd_pass    one pass of step 2^i, the 3x3 prefilter of v fused in: one pixel per lane, a wave = 64 pixels of a row, a block = 4 rows; the
//                9 + 25 taps are served by L2 like k_dn_pass's (a tap row of a wave is 1 KiB of colour + 2 KiB of guide, contiguous)
//   k_gd_finish  (filtered rgb, FRAME.a)
//   k_gd_select  include/pt_steer.h's rule over the final (c_K, v_K), T and the class: one flag byte per pixel, the active pixels counted with a
//                ballot popcount per wave, summed in LDS, one global atomic per block (pt_reproject.hip's k_reproject counts its kept pixels so)
//   k_dm_prep, k_dm_var, k_dm_finish, k_dm_select  include/pt_demod.h: the same four on the illumination mean / albedo, around the shared k_gd_pass
//   k_gd_fill    include/pt_fill.h: FRAME' = FRAME with every pixel nothing was rendered into reconstructed from the valid 5x5 neighbours of its
//                surface (the prep kernels' colour and guide of the real FRAME); the passes then run on FRAME' as they run on a frame
// Not under the bit-exact contract of the render path: __expf, sqrtf, and the summation order is the tap loop's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_device.hpp"

namespace {

constexpr int GD_BX = 64, GD_BY = 4;

__device__ __forceinline__ bool finite3(float a, float b, float c) { return __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c); }
__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
// max(x, 0) of the header: a NaN is no estimate
__device__ __forceinline__ float clampVar(float x) { return x >= 0.0f ? x : (x < 0.0f ? 0.0f : __builtin_inff()); }

__global__ void __launch_bounds__(256) k_gd_prep(const float4* frame, const float4* feat, int n, float4* col, float4* guide) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 F = frame[i], f0 = feat[4 * (size_t)i], f1 = feat[4 * (size_t)i + 1];
    const float a = F.w;
    const float mx = F.x / a, my = F.y / a, mz = F.z / a;
    const bool valid = a > 0.0f && finite3(mx, my, mz) && __builtin_isfinite(f0.x) && finite3(f0.y, f0.z, f0.w) && finite3(f1.x, f1.y, f1.z);
    const float cls = valid ? (__float_as_int(f1.w) >= 0 ? 1.0f : 2.0f) : 0.0f;
    col[i] = a > 0.0f ? make_float4(mx, my, mz, 0.0f) : make_float4(F.x, F.y, F.z, 0.0f);
    guide[2 * (size_t)i] = f0;
    guide[2 * (size_t)i + 1] = make_float4(f1.x, f1.y, f1.z, cls);
}

__global__ void __launch_bounds__(GD_BX * GD_BY) k_gd_var(const float4* __restrict__ frame, const float4* __restrict__ feat, const float4* __restrict__ stats,
                                                         const float4* __restrict__ guide, float4* __restrict__ col, int W, int H, float minFrames) {
    const int x = blockIdx.x * GD_BX + threadIdx.x, y = blockIdx.y * GD_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float cls = guide[2 * p + 1].w;
    if (cls == 0.0f) return;                                      // invalid: v is never read
    const float4 T = stats[p];
    float s2;
    if (T.z >= minFrames) {
        const float m = T.x / T.z;
        s2 = clampVar((T.y - T.x * m) / (T.z - 1.0f));
    } else {
        const bool hit = cls == 1.0f;
        const int mat = hit ? __float_as_int(feat[4 * p + 2].w) : 0;
        float S = 0.0f, Q = 0.0f, N = 0.0f;
        for (int dy = -3; dy <= 3; dy++) {
            const int yy = y + dy;
            if (yy < 0 || yy >= H) continue;
            for (int dx = -3; dx <= 3; dx++) {
                const int xx = x + dx;
                if (xx < 0 || xx >= W) continue;
                const size_t q = (size_t)yy * W + xx;
                if (guide[2 * q + 1].w != cls) continue;
                if (hit && __float_as_int(feat[4 * q + 2].w) != mat) continue;
                const float4 Tq = stats[q];
                if (!(Tq.z >= 1.0f)) continue;
                S = S + Tq.x; Q = Q + Tq.y; N = N + Tq.z;
            }
        }
        s2 = N >= 2.0f ? clampVar((Q - S * (S / N)) / (N - 1.0f)) : __builtin_inff();
    }
    reinterpret_cast<float*>(col + p)[3] = s2 / frame[p].w;
}

// inv = (1 / sn^2, 1 / sd^2, 1 / sa^2), each clamped to FLT_MAX; sigmaLum = +inf switches the luminance term off
__global__ void __launch_bounds__(GD_BX * GD_BY) k_gd_pass(const float4* __restrict__ in, const float4* __restrict__ guide, float4* __restrict__ out, int W, int H,
                                                          int step, float sigmaLum, float3 inv) {
    const int x = blockIdx.x * GD_BX + threadIdx.x, y = blockIdx.y * GD_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float4 cp = in[p];
    const float4 gp1 = guide[2 * p + 1];
    const float cls = gp1.w;
    if (cls == 0.0f) { out[p] = cp; return; }                     // invalid: passed through, weighs no neighbour
    const bool hit = cls == 1.0f;
    // g_p: the 3x3 binomial prefilter of v over p's valid neighbours of its class
    const float k3[3] = {0.25f, 0.5f, 0.25f};
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int xx = x + dx;
            if (xx < 0 || xx >= W) continue;
            const size_t q = (size_t)yy * W + xx;
            if (guide[2 * q + 1].w != cls) continue;
            const float k = k3[dy + 1] * k3[dx + 1];
            gs += k * in[q].w; gw += k;
        }
    }
    const float g = gs / gw;
    const bool lumOn = __builtin_isfinite(sigmaLum) && g != __builtin_inff();
    const float invDen = lumOn ? 1.0f / (sigmaLum * sqrtf(g) + 1e-10f) : 0.0f;
    const float lp = lum(cp.x, cp.y, cp.z);
    const float4 gp0 = hit ? guide[2 * p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float invT = 1.0f / gp0.x;
    const float h[5] = {1.0f / 16.0f, 4.0f / 16.0f, 6.0f / 16.0f, 4.0f / 16.0f, 1.0f / 16.0f};
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sv = 0.0f;
    bool vInf = false;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int yy = y + dy * step;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int xx = x + dx * step;
            if (xx < 0 || xx >= W) continue;
            const size_t q = (size_t)yy * W + xx;
            const float4 g1 = guide[2 * q + 1];
            if (g1.w != cls) continue;                            // invalid, or hit against miss
            const float4 cq = in[q];
            float e = lumOn ? __builtin_fabsf(lp - lum(cq.x, cq.y, cq.z)) * invDen : 0.0f;
            if (hit) {
                const float4 g0 = guide[2 * q];
                const float nx = gp0.y - g0.y, ny = gp0.z - g0.z, nz = gp0.w - g0.w;
                const float dt = (gp0.x - g0.x) * invT;
                const float ar = gp1.x - g1.x, ag = gp1.y - g1.y, ab = gp1.z - g1.z;
                e += (nx * nx + ny * ny + nz * nz) * inv.x + (dt * dt) * inv.y + (ar * ar + ag * ag + ab * ab) * inv.z;
            }
            const float w = (h[dy + 2] * h[dx + 2]) * __expf(-e);
            if (w < 1e-30f) continue;                             // the header's cut: __expf's underflow is no part of the rule
            sr += w * cq.x; sg += w * cq.y; sb += w * cq.z; sw += w;
            if (cq.w == __builtin_inff()) vInf = true;
            else sv += (w * w) * cq.w;
        }
    }
    out[p] = make_float4(sr / sw, sg / sw, sb / sw, vInf ? __builtin_inff() : sv / (sw * sw));
}

__global__ void __launch_bounds__(256) k_gd_finish(const float4* col, const float4* frame, int n, float4* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 c = col[i];
    out[i] = make_float4(c.x, c.y, c.z, frame[i].w);
}

// steps 1-5 of include/pt_steer.h.  cv: (c_K, v_K) per pixel; guide: k_gd_prep's (the class in the second record's w); mask: W*H bytes;
// count: zeroed by the caller.  rule = (rel_err, abs_err), ov = (mouse x, mouse y, resolution) of the overlay test.
__global__ void __launch_bounds__(GD_BX * GD_BY) k_gd_select(const float4* __restrict__ cv, const float4* __restrict__ stats, const float4* __restrict__ guide,
                                                            int W, int H, float minFrames, int maxFrames, float2 rule, float3 ov,
                                                            unsigned char* __restrict__ mask, unsigned* __restrict__ count) {
    __shared__ unsigned sCnt[GD_BY];
    const int x = blockIdx.x * GD_BX + threadIdx.x, y = blockIdx.y * GD_BY + threadIdx.y;
    bool on = false;
    if (x < W && y < H) {
        const size_t p = (size_t)y * W + x;
        ptd::FrameConst fc{};
        fc.mouse[0] = ov.x; fc.mouse[1] = ov.y; fc.resolution = ov.z;
        const float4 T = stats[p];
        const float n = T.z;
        if (ptd::inMouseOverlay(fc, x, y)) on = false;                                     // 1
        else if (maxFrames > 0 && n >= (float)maxFrames) on = false;                       // 2
        else if (n < minFrames) on = true;                                                 // 3
        else if (guide[2 * p + 1].w == 0.0f) {                                             // 4: invalid, the own-moment rule of include/pt_adaptive.h
            const float mean = T.x / n;
            const float var = (T.y - T.x * mean) / (n - 1.0f);
            const float err2 = var / n;
            const float tol = fmaxf(rule.x * fabsf(mean), rule.y);
            on = err2 > tol * tol;
        } else {                                                                           // 5: the filtered mean and its carried variance
            const float4 c = cv[p];
            const float tol = fmaxf(rule.x * fabsf(lum(c.x, c.y, c.z)), rule.y);
            on = c.w == __builtin_inff() || c.w > tol * tol;
        }
        mask[p] = on ? 1 : 0;
    }
    const unsigned long long b = __ballot(on);
    if (threadIdx.x == 0) sCnt[threadIdx.y] = (unsigned)__popcll(b);                      // a wave is one row of the block
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < GD_BY; w++) t += sCnt[w];
        if (t) atomicAdd(count, t);
    }
}

// ---- albedo demodulation (include/pt_demod.h): the same pipeline on the illumination I = c / a.  k_gd_pass runs unchanged on (I, v); the four
// kernels around it have a variant each.  The guide keeps the raw Kd (the albedo edge term compares it), so a pixel's a and L are recomputed
// from the 16-B guide record that gives its class: no further loads.

// a_p and L_p of the header from the second guide record (Kd, class): the floored Kd of a valid hit, (1, 1, 1) and exactly 1 otherwise
__device__ __forceinline__ float3 albedoOf(const float4 g1, float floorA) {
    return g1.w == 1.0f ? make_float3(fmaxf(g1.x, floorA), fmaxf(g1.y, floorA), fmaxf(g1.z, floorA)) : make_float3(1.0f, 1.0f, 1.0f);
}
__device__ __forceinline__ float albedoLum(const float4 g1, float floorA) {
    if (g1.w != 1.0f) return 1.0f;
    const float3 a = albedoOf(g1, floorA);
    return lum(a.x, a.y, a.z);
}

// k_gd_prep with I = mean / a in the colour record of a valid hit; a valid hit whose I is not finite becomes invalid (class 0, its mean passed through)
__global__ void __launch_bounds__(256) k_dm_prep(const float4* frame, const float4* feat, int n, float floorA, float4* col, float4* guide) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 F = frame[i], f0 = feat[4 * (size_t)i], f1 = feat[4 * (size_t)i + 1];
    const float a = F.w;
    const float mx = F.x / a, my = F.y / a, mz = F.z / a;
    bool valid = a > 0.0f && finite3(mx, my, mz) && __builtin_isfinite(f0.x) && finite3(f0.y, f0.z, f0.w) && finite3(f1.x, f1.y, f1.z);
    const bool hit = valid && __float_as_int(f1.w) >= 0;
    float4 c = a > 0.0f ? make_float4(mx, my, mz, 0.0f) : make_float4(F.x, F.y, F.z, 0.0f);
    if (hit) {
        const float ix = mx / fmaxf(f1.x, floorA), iy = my / fmaxf(f1.y, floorA), iz = mz / fmaxf(f1.z, floorA);
        if (finite3(ix, iy, iz)) c = make_float4(ix, iy, iz, 0.0f);
        else valid = false;
    }
    const float cls = valid ? (hit ? 1.0f : 2.0f) : 0.0f;
    col[i] = c;
    guide[2 * (size_t)i] = f0;
    guide[2 * (size_t)i + 1] = make_float4(f1.x, f1.y, f1.z, cls);
}

// k_gd_var on T' = (sY / L, (sYY / L) / L, n): the pixel's own L for its own moments, each tap's own L in the pooled sums
__global__ void __launch_bounds__(GD_BX * GD_BY) k_dm_var(const float4* __restrict__ frame, const float4* __restrict__ feat, const float4* __restrict__ stats,
                                                         const float4* __restrict__ guide, float4* __restrict__ col, int W, int H, float minFrames, float floorA) {
    const int x = blockIdx.x * GD_BX + threadIdx.x, y = blockIdx.y * GD_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float4 gp1 = guide[2 * p + 1];
    const float cls = gp1.w;
    if (cls == 0.0f) return;                                      // invalid: v is never read
    const bool hit = cls == 1.0f;
    const float4 T = stats[p];
    float s2;
    if (T.z >= minFrames) {
        float sY = T.x, sYY = T.y;
        if (hit) { const float L = albedoLum(gp1, floorA); sY = T.x / L; sYY = (T.y / L) / L; }
        const float m = sY / T.z;
        s2 = clampVar((sYY - sY * m) / (T.z - 1.0f));
    } else {
        const int mat = hit ? __float_as_int(feat[4 * p + 2].w) : 0;
        float S = 0.0f, Q = 0.0f, N = 0.0f;
        for (int dy = -3; dy <= 3; dy++) {
            const int yy = y + dy;
            if (yy < 0 || yy >= H) continue;
            for (int dx = -3; dx <= 3; dx++) {
                const int xx = x + dx;
                if (xx < 0 || xx >= W) continue;
                const size_t q = (size_t)yy * W + xx;
                const float4 gq1 = guide[2 * q + 1];
                if (gq1.w != cls) continue;
                if (hit && __float_as_int(feat[4 * q + 2].w) != mat) continue;
                const float4 Tq = stats[q];
                if (!(Tq.z >= 1.0f)) continue;
                float sY = Tq.x, sYY = Tq.y;
                if (hit) { const float L = albedoLum(gq1, floorA); sY = Tq.x / L; sYY = (Tq.y / L) / L; }
                S = S + sY; Q = Q + sYY; N = N + Tq.z;
            }
        }
        s2 = N >= 2.0f ? clampVar((Q - S * (S / N)) / (N - 1.0f)) : __builtin_inff();
    }
    reinterpret_cast<float*>(col + p)[3] = s2 / frame[p].w;
}

// k_gd_finish with the pixel's own albedo put back: (a_p * I_K, FRAME.a)
__global__ void __launch_bounds__(256) k_dm_finish(const float4* col, const float4* guide, const float4* frame, int n, float floorA, float4* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 c = col[i];
    const float3 a = albedoOf(guide[2 * (size_t)i + 1], floorA);
    out[i] = make_float4(a.x * c.x, a.y * c.y, a.z * c.z, frame[i].w);
}

// k_gd_select with include/pt_demod.h's step 5; steps 1-4 as there, on the raw T
__global__ void __launch_bounds__(GD_BX * GD_BY) k_dm_select(const float4* __restrict__ cv, const float4* __restrict__ stats, const float4* __restrict__ guide,
                                                            int W, int H, float minFrames, int maxFrames, float2 rule, float3 ov, float floorA,
                                                            unsigned char* __restrict__ mask, unsigned* __restrict__ count) {
    __shared__ unsigned sCnt[GD_BY];
    const int x = blockIdx.x * GD_BX + threadIdx.x, y = blockIdx.y * GD_BY + threadIdx.y;
    bool on = false;
    if (x < W && y < H) {
        const size_t p = (size_t)y * W + x;
        ptd::FrameConst fc{};
        fc.mouse[0] = ov.x; fc.mouse[1] = ov.y; fc.resolution = ov.z;
        const float4 T = stats[p];
        const float n = T.z;
        const float4 g1 = guide[2 * p + 1];
        if (ptd::inMouseOverlay(fc, x, y)) on = false;                                     // 1
        else if (maxFrames > 0 && n >= (float)maxFrames) on = false;                       // 2
        else if (n < minFrames) on = true;                                                 // 3
        else if (g1.w == 0.0f) {                                                           // 4: invalid, the own-moment rule of include/pt_adaptive.h
            const float mean = T.x / n;
            const float var = (T.y - T.x * mean) / (n - 1.0f);
            const float err2 = var / n;
            const float tol = fmaxf(rule.x * fabsf(mean), rule.y);
            on = err2 > tol * tol;
        } else {                                                                           // 5: the filtered colour, the variance brought back to colour
            const float4 c = cv[p];
            const float3 a = albedoOf(g1, floorA);
            const float tol = fmaxf(rule.x * fabsf(lum(a.x * c.x, a.y * c.y, a.z * c.z)), rule.y);
            float v = c.w;
            if (g1.w == 1.0f) { const float L = lum(a.x, a.y, a.z); v = (c.w * L) * L; }
            on = c.w == __builtin_inff() || v > tol * tol;
        }
        mask[p] = on ? 1 : 0;
    }
    const unsigned long long b = __ballot(on);
    if (threadIdx.x == 0) sCnt[threadIdx.y] = (unsigned)__popcll(b);                      // a wave is one row of the block
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < GD_BY; w++) t += sCnt[w];
        if (t) atomicAdd(count, t);
    }
}

// ---- the prefill of include/pt_fill.h: FRAME' for the pixels nothing was rendered into.  col, guide: k_gd_prep's (floorA == 0) or k_dm_prep's
// (floorA > 0) of the real FRAME, so col holds every source's x_q (mean or illumination) and the guide's class says which taps are valid; a hole
// is class 0 there, so its own hit or miss comes from the raw hit code.  Only holes read taps: the 24 of them are served by L2 like k_gd_pass's.
// inv as k_gd_pass's.  count: zeroed by the caller, the holes that found a source (counted as k_gd_select counts).
__global__ void __launch_bounds__(GD_BX * GD_BY) k_gd_fill(const float4* __restrict__ frame, const float4* __restrict__ feat, const float4* __restrict__ col,
                                                          const float4* __restrict__ guide, float4* __restrict__ out, int W, int H, float3 inv, float floorA,
                                                          unsigned* __restrict__ count) {
    __shared__ unsigned sCnt[GD_BY];
    const int x = blockIdx.x * GD_BX + threadIdx.x, y = blockIdx.y * GD_BY + threadIdx.y;
    bool filled = false;
    if (x < W && y < H) {
        const size_t p = (size_t)y * W + x;
        float4 F = frame[p];
        if (F.w <= 0.0f) {
            const float4 gp0 = guide[2 * p], gp1 = guide[2 * p + 1];
            if (__builtin_isfinite(gp0.x) && finite3(gp0.y, gp0.z, gp0.w) && finite3(gp1.x, gp1.y, gp1.z)) {
                const bool hit = __float_as_int(feat[4 * p + 1].w) >= 0;
                const float cls = hit ? 1.0f : 2.0f;
                const int mat = hit ? __float_as_int(feat[4 * p + 2].w) : 0;
                const float invT = 1.0f / gp0.x;
                const float h[5] = {1.0f / 16.0f, 4.0f / 16.0f, 6.0f / 16.0f, 4.0f / 16.0f, 1.0f / 16.0f};
                float sr = 0.0f, sg = 0.0f, sb = 0.0f, S = 0.0f, B = 0.0f;
#pragma unroll
                for (int dy = -2; dy <= 2; dy++) {
                    const int yy = y + dy;
                    if (yy < 0 || yy >= H) continue;
#pragma unroll
                    for (int dx = -2; dx <= 2; dx++) {
                        const int xx = x + dx;
                        if (xx < 0 || xx >= W || (dx == 0 && dy == 0)) continue;
                        const size_t q = (size_t)yy * W + xx;
                        const float4 g1 = guide[2 * q + 1];
                        if (g1.w != cls) continue;                // invalid (a hole included), or hit against miss
                        float w = h[dy + 2] * h[dx + 2];
                        if (hit) {
                            if (__float_as_int(feat[4 * q + 2].w) != mat) continue;
                            const float4 g0 = guide[2 * q];
                            const float nx = gp0.y - g0.y, ny = gp0.z - g0.z, nz = gp0.w - g0.w;
                            const float dt = (gp0.x - g0.x) * invT;
                            const float ar = gp1.x - g1.x, ag = gp1.y - g1.y, ab = gp1.z - g1.z;
                            const float e = (nx * nx + ny * ny + nz * nz) * inv.x + (dt * dt) * inv.y + (ar * ar + ag * ag + ab * ab) * inv.z;
                            w = w * __expf(-e);
                        }
                        if (w < 1e-30f) continue;
                        const float4 cq = col[q];
                        sr += w * cq.x; sg += w * cq.y; sb += w * cq.z; S += w;
                        B += (w * w) / frame[q].w;
                        filled = true;
                    }
                }
                if (filled) {
                    const float A = (S * S) / B;
                    const bool demod = hit && floorA > 0.0f;
                    const float ax = demod ? fmaxf(gp1.x, floorA) : 1.0f, ay = demod ? fmaxf(gp1.y, floorA) : 1.0f, az = demod ? fmaxf(gp1.z, floorA) : 1.0f;
                    F = make_float4((ax * (sr / S)) * A, (ay * (sg / S)) * A, (az * (sb / S)) * A, A);
                }
            }
        }
        out[p] = F;
    }
    const unsigned long long b = __ballot(filled);
    if (threadIdx.x == 0) sCnt[threadIdx.y] = (unsigned)__popcll(b);                      // a wave is one row of the block
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < GD_BY; w++) t += sCnt[w];
        if (t) atomicAdd(count, t);
    }
}

float clampInv(float v) { return v > 3.402823466e38f ? 3.402823466e38f : v; }

}  // namespace

// frame, stats: W*H float4 (FRAME and T in pixel order), feat: W*H*4 float4 (all read only); col0, col1: W*H float4 ping-pong; guide: 2*W*H float4;
// out: W*H float4.  sigma = (luminance, normal, depth, albedo) and minFrames already checked by the caller.  alpha: the image whose .a the output
// takes, nullptr = frame (include/pt_fill.h filters FRAME' and returns the real FRAME's count).  Enqueued on `s`; returns the first launch error.
hipError_t guidedLaunch(const float4* frame, const float4* feat, const float4* stats, int W, int H, int iterations, const float sigma[4], int minFrames,
                        float4* col0, float4* col1, float4* guide, float4* out, hipStream_t s, const float4* alpha) {
    const int n = W * H;
    const dim3 lin((unsigned)((n + 255) / 256));
    const dim3 grid((unsigned)((W + GD_BX - 1) / GD_BX), (unsigned)((H + GD_BY - 1) / GD_BY));
    hipLaunchKernelGGL(k_gd_prep, lin, dim3(256), 0, s, frame, feat, n, col0, guide);
    float4* src = col0;
    float4* dst = col1;
    if (iterations > 0) {
        hipLaunchKernelGGL(k_gd_var, grid, dim3(GD_BX, GD_BY), 0, s, frame, feat, stats, guide, col0, W, H, (float)minFrames);
        const float3 inv = make_float3(clampInv(1.0f / (sigma[1] * sigma[1])), clampInv(1.0f / (sigma[2] * sigma[2])), clampInv(1.0f / (sigma[3] * sigma[3])));
        for (int i = 0; i < iterations; i++) {
            hipLaunchKernelGGL(k_gd_pass, grid, dim3(GD_BX, GD_BY), 0, s, src, guide, dst, W, H, 1 << i, sigma[0], inv);
            float4* t = src; src = dst; dst = t;
        }
    }
    hipLaunchKernelGGL(k_gd_finish, lin, dim3(256), 0, s, src, alpha ? alpha : frame, n, out);
    return hipGetLastError();
}

// include/pt_steer.h's selection: k_gd_prep, k_gd_var (always, K = 0 included), K passes, k_gd_select into mask[W*H] and *count (zeroed here).
// Arguments as guidedLaunch's; rule = (rel_err, abs_err), ov = (mouse x, mouse y, resolution), all checked by the caller.  Enqueued on `s`;
// returns the first launch error.
hipError_t guidedSelectLaunch(const float4* frame, const float4* feat, const float4* stats, int W, int H, int iterations, const float sigma[4], int minFrames,
                              int maxFrames, const float rule[2], const float ov[3], float4* col0, float4* col1, float4* guide, unsigned char* mask,
                              unsigned* count, hipStream_t s) {
    const int n = W * H;
    const dim3 lin((unsigned)((n + 255) / 256));
    const dim3 grid((unsigned)((W + GD_BX - 1) / GD_BX), (unsigned)((H + GD_BY - 1) / GD_BY));
    hipError_t e = hipMemsetAsync(count, 0, 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_gd_prep, lin, dim3(256), 0, s, frame, feat, n, col0, guide);
    hipLaunchKernelGGL(k_gd_var, grid, dim3(GD_BX, GD_BY), 0, s, frame, feat, stats, guide, col0, W, H, (float)minFrames);
    const float3 inv = make_float3(clampInv(1.0f / (sigma[1] * sigma[1])), clampInv(1.0f / (sigma[2] * sigma[2])), clampInv(1.0f / (sigma[3] * sigma[3])));
    float4* src = col0;
    float4* dst = col1;
    for (int i = 0; i < iterations; i++) {
        hipLaunchKernelGGL(k_gd_pass, grid, dim3(GD_BX, GD_BY), 0, s, src, guide, dst, W, H, 1 << i, sigma[0], inv);
        float4* t = src; src = dst; dst = t;
    }
    hipLaunchKernelGGL(k_gd_select, grid, dim3(GD_BX, GD_BY), 0, s, src, stats, guide, W, H, (float)minFrames, maxFrames, make_float2(rule[0], rule[1]),
                       make_float3(ov[0], ov[1], ov[2]), mask, count);
    return hipGetLastError();
}

// include/pt_demod.h's filter: guidedLaunch with k_dm_prep, k_dm_var and k_dm_finish around the shared passes.  floorA = albedo_floor, checked by
// the caller; the other arguments as guidedLaunch's.
hipError_t guidedDemodLaunch(const float4* frame, const float4* feat, const float4* stats, int W, int H, int iterations, const float sigma[4], int minFrames,
                             float floorA, float4* col0, float4* col1, float4* guide, float4* out, hipStream_t s, const float4* alpha) {
    const int n = W * H;
    const dim3 lin((unsigned)((n + 255) / 256));
    const dim3 grid((unsigned)((W + GD_BX - 1) / GD_BX), (unsigned)((H + GD_BY - 1) / GD_BY));
    hipLaunchKernelGGL(k_dm_prep, lin, dim3(256), 0, s, frame, feat, n, floorA, col0, guide);
    float4* src = col0;
    float4* dst = col1;
    if (iterations > 0) {
        hipLaunchKernelGGL(k_dm_var, grid, dim3(GD_BX, GD_BY), 0, s, frame, feat, stats, guide, col0, W, H, (float)minFrames, floorA);
        const float3 inv = make_float3(clampInv(1.0f / (sigma[1] * sigma[1])), clampInv(1.0f / (sigma[2] * sigma[2])), clampInv(1.0f / (sigma[3] * sigma[3])));
        for (int i = 0; i < iterations; i++) {
            hipLaunchKernelGGL(k_gd_pass, grid, dim3(GD_BX, GD_BY), 0, s, src, guide, dst, W, H, 1 << i, sigma[0], inv);
            float4* t = src; src = dst; dst = t;
        }
    }
    hipLaunchKernelGGL(k_dm_finish, lin, dim3(256), 0, s, src, guide, alpha ? alpha : frame, n, floorA, out);
    return hipGetLastError();
}

// include/pt_demod.h's selection: guidedSelectLaunch with k_dm_prep, k_dm_var and k_dm_select around the shared passes.
hipError_t guidedDemodSelectLaunch(const float4* frame, const float4* feat, const float4* stats, int W, int H, int iterations, const float sigma[4],
                                   int minFrames, int maxFrames, const float rule[2], const float ov[3], float floorA, float4* col0, float4* col1,
                                   float4* guide, unsigned char* mask, unsigned* count, hipStream_t s) {
    const int n = W * H;
    const dim3 lin((unsigned)((n + 255) / 256));
    const dim3 grid((unsigned)((W + GD_BX - 1) / GD_BX), (unsigned)((H + GD_BY - 1) / GD_BY));
    hipError_t e = hipMemsetAsync(count, 0, 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_dm_prep, lin, dim3(256), 0, s, frame, feat, n, floorA, col0, guide);
    hipLaunchKernelGGL(k_dm_var, grid, dim3(GD_BX, GD_BY), 0, s, frame, feat, stats, guide, col0, W, H, (float)minFrames, floorA);
    const float3 inv = make_float3(clampInv(1.0f / (sigma[1] * sigma[1])), clampInv(1.0f / (sigma[2] * sigma[2])), clampInv(1.0f / (sigma[3] * sigma[3])));
    float4* src = col0;
    float4* dst = col1;
    for (int i = 0; i < iterations; i++) {
        hipLaunchKernelGGL(k_gd_pass, grid, dim3(GD_BX, GD_BY), 0, s, src, guide, dst, W, H, 1 << i, sigma[0], inv);
        float4* t = src; src = dst; dst = t;
    }
    hipLaunchKernelGGL(k_dm_select, grid, dim3(GD_BX, GD_BY), 0, s, src, stats, guide, W, H, (float)minFrames, maxFrames, make_float2(rule[0], rule[1]),
                       make_float3(ov[0], ov[1], ov[2]), floorA, mask, count);
    return hipGetLastError();
}

// include/pt_fill.h's FRAME' into fill[W*H]: the prep kernel of the rule floorA selects (0: k_gd_prep, > 0: k_dm_prep) on the real FRAME, then
// k_gd_fill; *count (zeroed here) = the holes filled.  sigma as guidedLaunch's (its luminance entry unused); col0, guide: scratch, free afterwards.
hipError_t fillLaunch(const float4* frame, const float4* feat, int W, int H, const float sigma[4], float floorA, float4* col0, float4* guide, float4* fill,
                      unsigned* count, hipStream_t s) {
    const int n = W * H;
    const dim3 lin((unsigned)((n + 255) / 256));
    const dim3 grid((unsigned)((W + GD_BX - 1) / GD_BX), (unsigned)((H + GD_BY - 1) / GD_BY));
    hipError_t e = hipMemsetAsync(count, 0, 4, s);
    if (e != hipSuccess) return e;
    if (floorA > 0.0f) hipLaunchKernelGGL(k_dm_prep, lin, dim3(256), 0, s, frame, feat, n, floorA, col0, guide);
    else hipLaunchKernelGGL(k_gd_prep, lin, dim3(256), 0, s, frame, feat, n, col0, guide);
    const float3 inv = make_float3(clampInv(1.0f / (sigma[1] * sigma[1])), clampInv(1.0f / (sigma[2] * sigma[2])), clampInv(1.0f / (sigma[3] * sigma[3])));
    hipLaunchKernelGGL(k_gd_fill, grid, dim3(GD_BX, GD_BY), 0, s, frame, feat, (const float4*)col0, (const float4*)guide, fill, W, H, inv, floorA, count);
    return hipGetLastError();
}

// include/pt_fill.h's filtered image: fillLaunch, then guidedLaunch (floorA == 0) or guidedDemodLaunch on FRAME' in place of the frame, the output's
// alpha from the real FRAME.  Arguments as theirs; fill, count as fillLaunch's.
hipError_t guidedFilledLaunch(const float4* frame, const float4* feat, const float4* stats, int W, int H, int iterations, const float sigma[4], int minFrames,
                              float floorA, float4* col0, float4* col1, float4* guide, float4* fill, float4* out, unsigned* count, hipStream_t s) {
    const hipError_t e = fillLaunch(frame, feat, W, H, sigma, floorA, col0, guide, fill, count, s);
    if (e != hipSuccess) return e;
    if (floorA > 0.0f) return guidedDemodLaunch(fill, feat, stats, W, H, iterations, sigma, minFrames, floorA, col0, col1, guide, out, s, frame);
    return guidedLaunch(fill, feat, stats, W, H, iterations, sigma, minFrames, col0, col1, guide, out, s, frame);
}
