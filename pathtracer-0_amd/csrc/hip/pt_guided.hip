// pt_guided.hip — the variance-guided filter of include/pt_guided.h (the spatial half of Schied et al. 2017) for gfx950.
//
// Device pointers only: pt_hip.hip owns the buffers (the a-trous filter's scratch, shared), computes the feature records, brings T into pixel
// order and calls guidedLaunch on its stream.  A demodulated kernel (include/pt_demod.h, floorA > 0) is the DEMOD specialisation of the plain one's
// template or body wherever that left both kernels' code as it was (the prep kernels stay two); each keeps an argument list of its own, because
// the kernarg layout is part of its code.
//   k_gd_prep    per pixel: the mean FRAME.rgb / FRAME.a (raw rgb when FRAME.a <= 0) and the guide (t, N), (Kd, class) packed into 32 B, the
//                pixel's class (0 invalid, 1 hit, 2 miss) in the second record's w
//   k_gd_var     per pixel: the variance of the mean v = s2 / FRAME.a into the colour record's w; s2 from the pixel's own moments, or pooled
//                over its 7x7 window (same class, same material) when it has fewer than min_frames
//   k_gd_pass    one pass of step 2^i, the 3x3 prefilter of v fused in: one pixel per lane, a wave = 64 pixels of a row, a block = 4 rows; the
//                9 + 25 taps are served by L2 like k_dn_pass's (a tap row of a wave is 1 KiB of colour + 2 KiB of guide, contiguous)
//   k_gd_finish  (filtered rgb, FRAME.a)
//   k_gd_select  include/pt_steer.h's rule over the final (c_K, v_K), T and the class: one flag byte per pixel, the active pixels counted with a
//                ballot popcount per wave, summed in LDS, one global atomic per block (pt_reproject.hip's k_reproject counts its kept pixels so)
//   k_gd_prep_demod, k_gd_var<true>, k_gd_finish_demod, k_gd_select<true>  include/pt_demod.h: the same four on the illumination mean / albedo,
//                around the shared k_gd_pass
//   k_gd_fill    include/pt_fill.h: FRAME' = FRAME with every pixel nothing was rendered into reconstructed from the valid 5x5 neighbours of its
//                surface (the prep kernels' colour and guide of the real FRAME); the passes then run on FRAME' as they run on a frame
// Not under the bit-exact contract of the render path: __expf, sqrtf, and the summation order is the tap loop's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_device.hpp"
#include "pt_image_launch.hpp"

namespace {

constexpr int GD_BX = 64, GD_BY = 4;

__device__ __forceinline__ bool finite3(float a, float b, float c) { return __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c); }
__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
// max(x, 0) of the header: a NaN is no estimate
__device__ __forceinline__ float clampVar(float x) { return x >= 0.0f ? x : (x < 0.0f ? 0.0f : __builtin_inff()); }

// ---- albedo demodulation (include/pt_demod.h): the same pipeline on the illumination I = c / a.  k_gd_pass runs unchanged on (I, v); the
// kernels around it have a demodulated form.  The guide keeps the raw Kd (the albedo edge term compares it), so a pixel's a and L are recomputed from the 16-B
// guide record that gives its class: no further loads.

// a_p and L_p of the header from the second guide record (Kd, class): the floored Kd of a valid hit, (1, 1, 1) and exactly 1 otherwise
__device__ __forceinline__ float3 albedoOf(const float4 g1, float floorA) {
    return g1.w == 1.0f ? make_float3(fmaxf(g1.x, floorA), fmaxf(g1.y, floorA), fmaxf(g1.z, floorA)) : make_float3(1.0f, 1.0f, 1.0f);
}
__device__ __forceinline__ float albedoLum(const float4 g1, float floorA) {
    if (g1.w != 1.0f) return 1.0f;
    const float3 a = albedoOf(g1, floorA);
    return lum(a.x, a.y, a.z);
}
// Own: the argument the demodulated specialisation of a kernel has of its own, (floorA); the plain one has none, so that each keeps its kernarg layout
__device__ __forceinline__ float floorOf() { return 0.0f; }
__device__ __forceinline__ float floorOf(float floorA) { return floorA; }
// the second guide record of pixel p: all of it where the albedo is needed (DEMOD), else the 4 B of its class alone
template <bool DEMOD>
__device__ __forceinline__ float4 classRecord(const float4* __restrict__ guide, size_t p) {
    if (DEMOD) return guide[2 * p + 1];
    return make_float4(0.0f, 0.0f, 0.0f, guide[2 * p + 1].w);
}

// (Two kernels: every shared form of them that was tried moved instructions in the plain one.)
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
// k_gd_prep with I = mean / a in the colour record of a valid hit; a valid hit whose I is not finite becomes invalid (class 0, its mean passed through)
__global__ void __launch_bounds__(256) k_gd_prep_demod(const float4* frame, const float4* feat, int n, float floorA, float4* col, float4* guide) {
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

// s2 of the moments S = sum Y, Q = sum Y^2 over N frames
__device__ __forceinline__ float sampleVar(float S, float Q, float N) { return clampVar((Q - S * (S / N)) / (N - 1.0f)); }

// DEMOD: on T' = (sY / L, (sYY / L) / L, n), the pixel's own L for its own moments, each tap's own L in the pooled sums
template <bool DEMOD, class... Own>
__global__ void __launch_bounds__(GD_BX * GD_BY) k_gd_var(const float4* __restrict__ frame, const float4* __restrict__ feat, const float4* __restrict__ stats,
                                                         const float4* __restrict__ guide, float4* __restrict__ col, int W, int H, float minFrames, Own... own) {
    const float floorA = floorOf(own...);
    const int x = blockIdx.x * GD_BX + threadIdx.x, y = blockIdx.y * GD_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float4 gp1 = classRecord<DEMOD>(guide, p);
    const float cls = gp1.w;
    if (cls == 0.0f) return;                                      // invalid: v is never read
    const bool hit = cls == 1.0f;
    const bool scaled = DEMOD && hit;                             // the moments over the albedo luminance
    const float4 T = stats[p];
    float s2;
    if (T.z >= minFrames) {
        float sY = T.x, sYY = T.y;
        if (scaled) { const float L = albedoLum(gp1, floorA); sY = T.x / L; sYY = (T.y / L) / L; }
        s2 = sampleVar(sY, sYY, T.z);
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
                const float4 gq1 = classRecord<DEMOD>(guide, q);
                if (gq1.w != cls) continue;
                if (hit && __float_as_int(feat[4 * q + 2].w) != mat) continue;
                const float4 Tq = stats[q];
                if (!(Tq.z >= 1.0f)) continue;
                float sY = Tq.x, sYY = Tq.y;
                if (scaled) { const float L = albedoLum(gq1, floorA); sY = Tq.x / L; sYY = (Tq.y / L) / L; }
                S = S + sY; Q = Q + sYY; N = N + Tq.z;
            }
        }
        s2 = N >= 2.0f ? sampleVar(S, Q, N) : __builtin_inff();
    }
    reinterpret_cast<float*>(col + p)[3] = s2 / frame[p].w;
}
// the edge-stopping term of a hit p against its tap q: normal, relative depth and albedo, from the two guide records of each.
// inv = (1 / sn^2, 1 / sd^2, 1 / sa^2), each clamped to FLT_MAX; invT = 1 / t_p
__device__ __forceinline__ float edgeTerm(const float4& gp0, const float4& gp1, const float4& g0, const float4& g1, float invT, const float3& inv) {
    const float nx = gp0.y - g0.y, ny = gp0.z - g0.z, nz = gp0.w - g0.w;
    const float dt = (gp0.x - g0.x) * invT;
    const float ar = gp1.x - g1.x, ag = gp1.y - g1.y, ab = gp1.z - g1.z;
    return (nx * nx + ny * ny + nz * nz) * inv.x + (dt * dt) * inv.y + (ar * ar + ag * ag + ab * ab) * inv.z;
}

// inv as edgeTerm's; sigmaLum = +inf switches the luminance term off
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
                e += edgeTerm(gp0, gp1, g0, g1, invT, inv);
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

// (filtered rgb, FRAME.a); DEMOD: with the pixel's own albedo put back, (a_p * I_K, FRAME.a).  (The demodulated kernel's own arguments stand in two
// places, so the two share a body, not a template.)
template <bool DEMOD>
__device__ __forceinline__ void finishPixel(const float4* col, const float4* guide, const float4* frame, int n, float floorA, float4* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 c = col[i];
    const float3 a = DEMOD ? albedoOf(guide[2 * (size_t)i + 1], floorA) : make_float3(1.0f, 1.0f, 1.0f);
    out[i] = DEMOD ? make_float4(a.x * c.x, a.y * c.y, a.z * c.z, frame[i].w) : make_float4(c.x, c.y, c.z, frame[i].w);
}
__global__ void __launch_bounds__(256) k_gd_finish(const float4* col, const float4* frame, int n, float4* out) {
    finishPixel<false>(col, nullptr, frame, n, 0.0f, out);
}
__global__ void __launch_bounds__(256) k_gd_finish_demod(const float4* col, const float4* guide, const float4* frame, int n, float floorA, float4* out) {
    finishPixel<true>(col, guide, frame, n, floorA, out);
}

// steps 1-5 of include/pt_steer.h.  cv: (c_K, v_K) per pixel; guide: the prep kernel's (the class in the second record's w); mask: W*H bytes;
// count: zeroed by the caller.  rule = (rel_err, abs_err), ov = (mouse x, mouse y, resolution) of the overlay test.
// DEMOD: include/pt_demod.h's step 5; steps 1-4 as they are, on the raw T
template <bool DEMOD, class... Own>
__global__ void __launch_bounds__(GD_BX * GD_BY) k_gd_select(const float4* __restrict__ cv, const float4* __restrict__ stats, const float4* __restrict__ guide,
                                                            int W, int H, float minFrames, int maxFrames, float2 rule, float3 ov, Own... own,
                                                            unsigned char* __restrict__ mask, unsigned* __restrict__ count) {
    __shared__ unsigned sCnt[GD_BY];
    const float floorA = floorOf(own...);
    const int x = blockIdx.x * GD_BX + threadIdx.x, y = blockIdx.y * GD_BY + threadIdx.y;
    bool on = false;
    if (x < W && y < H) {
        const size_t p = (size_t)y * W + x;
        ptd::FrameConst fc{};
        fc.mouse[0] = ov.x; fc.mouse[1] = ov.y; fc.resolution = ov.z;
        const float4 T = stats[p];
        const float n = T.z;
        float4 g1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (DEMOD) g1 = guide[2 * p + 1];                                                  // (the plain rule reads the class alone, in step 4)
        if (ptd::inMouseOverlay(fc, x, y)) on = false;                                     // 1
        else if (maxFrames > 0 && n >= (float)maxFrames) on = false;                       // 2
        else if (n < minFrames) on = true;                                                 // 3
        else if ((DEMOD ? g1.w : guide[2 * p + 1].w) == 0.0f) {                            // 4: invalid, the own-moment rule of include/pt_adaptive.h
            const float mean = T.x / n;
            const float var = (T.y - T.x * mean) / (n - 1.0f);
            const float err2 = var / n;
            const float tol = fmaxf(rule.x * fabsf(mean), rule.y);
            on = err2 > tol * tol;
        } else if (DEMOD) {                                                                // 5: the filtered colour, the variance brought back to colour
            const float4 c = cv[p];
            const float3 a = albedoOf(g1, floorA);
            const float tol = fmaxf(rule.x * fabsf(lum(a.x * c.x, a.y * c.y, a.z * c.z)), rule.y);
            float v = c.w;
            if (g1.w == 1.0f) { const float L = lum(a.x, a.y, a.z); v = (c.w * L) * L; }
            on = c.w == __builtin_inff() || v > tol * tol;
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

// ---- the prefill of include/pt_fill.h: FRAME' for the pixels nothing was rendered into.  col, guide: the prep kernel's (plain when floorA == 0, demodulated
// when > 0) of the real FRAME, so col holds every source's x_q (mean or illumination) and the guide's class says which taps are valid; a hole
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
                            w = w * __expf(-edgeTerm(gp0, gp1, g0, g1, invT, inv));
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

// The launches a job enqueues, in order: with `fill`, the memset of its count, the prep kernel on the real FRAME and k_gd_fill (FRAME' is the frame
// from there on); for a selection the memset of its count; then prep, k_gd_var (the filter: when iterations > 0; the selection: always, K = 0
// included), the K passes, and the finish kernel (its alpha the real FRAME's: include/pt_fill.h returns the real count) or the select kernel.
// floorA > 0 picks the demodulated kernel of every pair, and nothing else does.
hipError_t guidedLaunch(const GuidedJob& j, hipStream_t s) {
    const int W = j.W, H = j.H, n = W * H;
    const dim3 lin((unsigned)((n + 255) / 256)), blk(GD_BX, GD_BY);
    const dim3 grid((unsigned)((W + GD_BX - 1) / GD_BX), (unsigned)((H + GD_BY - 1) / GD_BY));
    const bool demod = j.floorA > 0.0f;
    const float3 inv = make_float3(clampInv(1.0f / (j.sigma[1] * j.sigma[1])), clampInv(1.0f / (j.sigma[2] * j.sigma[2])), clampInv(1.0f / (j.sigma[3] * j.sigma[3])));
    auto prep = [&](const float4* frame) {
        if (demod) hipLaunchKernelGGL(k_gd_prep_demod, lin, dim3(256), 0, s, frame, j.feat, n, j.floorA, j.col0, j.guide);
        else hipLaunchKernelGGL(k_gd_prep, lin, dim3(256), 0, s, frame, j.feat, n, j.col0, j.guide);
    };
    const float4* frame = j.frame;
    if (j.fill) {
        hipError_t e = hipMemsetAsync(j.fillCount, 0, 4, s);
        if (e != hipSuccess) return e;
        prep(j.frame);
        hipLaunchKernelGGL(k_gd_fill, grid, blk, 0, s, j.frame, j.feat, (const float4*)j.col0, (const float4*)j.guide, j.fill, W, H, inv, j.floorA, j.fillCount);
        e = hipGetLastError();
        if (e != hipSuccess || !(j.out || j.mask)) return e;
        frame = j.fill;
    }
    if (j.mask) {
        const hipError_t e = hipMemsetAsync(j.count, 0, 4, s);
        if (e != hipSuccess) return e;
    }
    prep(frame);
    float4* src = j.col0;
    float4* dst = j.col1;
    if (j.mask || j.iterations > 0) {
        if (demod) hipLaunchKernelGGL((k_gd_var<true, float>), grid, blk, 0, s, frame, j.feat, j.stats, j.guide, j.col0, W, H, (float)j.minFrames, j.floorA);
        else hipLaunchKernelGGL((k_gd_var<false>), grid, blk, 0, s, frame, j.feat, j.stats, j.guide, j.col0, W, H, (float)j.minFrames);
        for (int i = 0; i < j.iterations; i++) {
            hipLaunchKernelGGL(k_gd_pass, grid, blk, 0, s, src, j.guide, dst, W, H, 1 << i, j.sigma[0], inv);
            float4* t = src; src = dst; dst = t;
        }
    }
    if (j.mask) {
        const float2 rule = make_float2(j.relErr, j.absErr);
        const float3 ov = make_float3(j.overlay[0], j.overlay[1], j.overlay[2]);
        if (demod) hipLaunchKernelGGL((k_gd_select<true, float>), grid, blk, 0, s, src, j.stats, j.guide, W, H, (float)j.minFrames, j.maxFrames, rule, ov, j.floorA, j.mask, j.count);
        else hipLaunchKernelGGL((k_gd_select<false>), grid, blk, 0, s, src, j.stats, j.guide, W, H, (float)j.minFrames, j.maxFrames, rule, ov, j.mask, j.count);
    } else if (demod) {
        hipLaunchKernelGGL(k_gd_finish_demod, lin, dim3(256), 0, s, src, j.guide, j.frame, n, j.floorA, j.out);
    } else {
        hipLaunchKernelGGL(k_gd_finish, lin, dim3(256), 0, s, src, j.frame, n, j.out);
    }
    return hipGetLastError();
}
