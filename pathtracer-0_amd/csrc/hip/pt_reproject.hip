// pt_reproject.hip — the reprojection of include/pt_reproject.h for gfx950.
//
// Device pointers only: pt_hip.hip owns the buffers, computes both sets of feature records and calls reprojectLaunch on its stream.
//   k_reproject  one lane per new pixel, a wave = 64 pixels of a row, a block = 16 rows.  Reads 48 B of Rn[p] (F0, F1.w, F2), the same of
//                Rh[s] at the source pixel (a near-identity gather for small moves: the rows of a wave stay together), then FRAME[s] and
//                T[s]; writes the new pixel of FRAME and T into scratch images.  The kept pixels are counted with a ballot popcount per
//                wave, summed in LDS, and one global atomic per block (one per wave, 32400 on one address at 1080p, cost 0.36 ms).
// Under the bit-exact contract: binary32 * + / sqrt in the header's order, no contraction (the build's -ffp-contract=off, IEEE divides).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_device.hpp"

using namespace ptd;

namespace {

constexpr int RP_BX = 64, RP_BY = 16;

struct ReprojCam {
    float On[3];                        // the current ORIGIN (the origin of Rn's rays)
    float mouseX, mouseY, resolution;   // the current mouse overlay
};
struct ReprojRule { float maxHistory, depthTol, normalTol; int allMaterials; };

__device__ __forceinline__ bool finite3(float a, float b, float c) { return __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c); }

__global__ void __launch_bounds__(RP_BX * RP_BY) k_reproject(const float4* __restrict__ rn, const float4* __restrict__ rh, const float4* __restrict__ frame,
                                                            const float4* __restrict__ stats, const FrameConst* __restrict__ hc, const unsigned char* __restrict__ matVD,
                                                            int nMat, int W, int H,
                                                            ReprojCam cam, ReprojRule r, float4* __restrict__ outFrame, float4* __restrict__ outStats,
                                                            unsigned* __restrict__ kept) {
    __shared__ unsigned blockKept;
    if (threadIdx.x == 0 && threadIdx.y == 0) blockKept = 0;
    __syncthreads();
    const int x = blockIdx.x * RP_BX + threadIdx.x, y = blockIdx.y * RP_BY + threadIdx.y;
    const bool in = x < W && y < H;
    const size_t p = (size_t)y * W + x;
    bool keep = false;
    float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f, f3 = 0.0f, t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;      // the kept FRAME and T (scalars: no stack copy)
    const float* M = hc->camRot;                                                           // the image's camera, as k_frame_setup built it
    const float O0 = hc->origin[0], O1 = hc->origin[1], O2 = hc->origin[2], ss = hc->screenSize, fl = hc->focalLength, hr = hc->screenHratio;
    FrameConst fc;
    fc.mouse[0] = cam.mouseX; fc.mouse[1] = cam.mouseY; fc.resolution = cam.resolution;
    if (in && !inMouseOverlay(fc, x, y)) {                                                 // 1
        const float4 n0 = rn[4 * p], n2 = rn[4 * p + 2];
        const int code = __float_as_int(reinterpret_cast<const float*>(rn + 4 * p + 1)[3]);
        const bool hit = code != -1;                                                       // 2
        const int mat = __float_as_int(n2.w);
        bool ok;
        float vx, vy, vz;
        if (hit) {
            ok = __builtin_isfinite(n0.x) && finite3(n0.y, n0.z, n0.w) && finite3(n2.x, n2.y, n2.z) && (unsigned)mat < (unsigned)nMat &&
                 (r.allMaterials || !matVD[mat]);
            vx = (cam.On[0] + n0.x * n2.x) - O0; vy = (cam.On[1] + n0.x * n2.y) - O1; vz = (cam.On[2] + n0.x * n2.z) - O2;
        } else {
            ok = true;
            vx = n2.x; vy = n2.y; vz = n2.z;
        }
        const float q0 = (vx * M[0] + vy * M[1]) + vz * M[2];                                  // 3
        const float q1 = (vx * M[3] + vy * M[4]) + vz * M[5];
        const float q2 = (vx * M[6] + vy * M[7]) + vz * M[8];
        const float a = (q0 / q2) * fl, b = (q1 / q2) * fl;                                   // 4
        const float sx = ((1.0f - a / ss) * 0.5f) * (float)W, sy = ((1.0f + b / (hr * ss)) * 0.5f) * (float)H;
        ok = ok && q2 > 0.0f && sx >= 0.0f && sx < (float)W && sy >= 0.0f && sy < (float)H;
        if (ok) {
            const size_t s = (size_t)(int)sy * W + (int)sx;
            const float4 h0 = rh[4 * s], h2 = rh[4 * s + 2];
            const bool hhit = __float_as_int(reinterpret_cast<const float*>(rh + 4 * s + 1)[3]) != -1;      // 5
            if (hit) {
                const float len = sqrtf((vx * vx + vy * vy) + vz * vz);
                ok = hhit && __float_as_int(h2.w) == mat && __builtin_isfinite(h0.x) && h0.x > 0.0f && __builtin_fabsf(len - h0.x) <= r.depthTol * h0.x &&
                     (n0.y * h0.y + n0.z * h0.z) + n0.w * h0.w >= r.normalTol;
            } else {
                ok = !hhit;
            }
            if (ok) {
                const float4 F = frame[s];                                                 // 6
                ok = F.w > 0.0f && finite3(F.x, F.y, F.z);
                if (ok) {                                                                  // 7
                    f0 = F.x; f1 = F.y; f2 = F.z; f3 = F.w;
                    if (F.w > r.maxHistory) { const float f = r.maxHistory / F.w; f0 = F.x * f; f1 = F.y * f; f2 = F.z * f; f3 = r.maxHistory; }
                    if (stats) {
                        const float4 T = stats[s];
                        t0 = T.x; t1 = T.y; t2 = T.z; t3 = T.w;
                        if (T.z > r.maxHistory) { const float g = r.maxHistory / T.z; t0 = T.x * g; t1 = T.y * g; t2 = r.maxHistory; }
                    }
                }
            }
        }
        keep = ok;
    }
    if (in) {
        outFrame[p] = keep ? make_float4(f0, f1, f2, f3) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (outStats) outStats[p] = keep ? make_float4(t0, t1, t2, t3) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const unsigned long long m = __ballot(keep);                                           // every lane of the block, in range or not
    if (threadIdx.x == 0 && m) atomicAdd(&blockKept, (unsigned)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0 && blockKept) atomicAdd(kept, blockKept);
}

// ---- include/pt_demod.h: the same mapping carrying illumination.  b of the header: the floored Kd of a record that is a hit (code != -1) with a
// finite Kd, else (1, 1, 1).  Kd is F1.xyz of the 64-B record whose hit code (F1.w) k_reproject reads anyway: one 16-B load instead of a 4-B one.
__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ float3 carriedAlbedo(const float4 f1, float floorA) {
    return __float_as_int(f1.w) != -1 && finite3(f1.x, f1.y, f1.z) ? make_float3(fmaxf(f1.x, floorA), fmaxf(f1.y, floorA), fmaxf(f1.z, floorA))
                                                                  : make_float3(1.0f, 1.0f, 1.0f);
}

// k_reproject, steps 1-6 line for line (a copy, so that k_reproject's own code stays what it was); step 7 scales F by b_n[p] / b_h[s] and T by
// rho = l(b_n[p]) / l(b_h[s]) before the caps
__global__ void __launch_bounds__(RP_BX * RP_BY) k_reproject_demod(const float4* __restrict__ rn, const float4* __restrict__ rh, const float4* __restrict__ frame,
                                                                  const float4* __restrict__ stats, const FrameConst* __restrict__ hc,
                                                                  const unsigned char* __restrict__ matVD, int nMat, int W, int H, ReprojCam cam, ReprojRule r,
                                                                  float floorA, float4* __restrict__ outFrame, float4* __restrict__ outStats,
                                                                  unsigned* __restrict__ kept) {
    __shared__ unsigned blockKept;
    if (threadIdx.x == 0 && threadIdx.y == 0) blockKept = 0;
    __syncthreads();
    const int x = blockIdx.x * RP_BX + threadIdx.x, y = blockIdx.y * RP_BY + threadIdx.y;
    const bool in = x < W && y < H;
    const size_t p = (size_t)y * W + x;
    bool keep = false;
    float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f, f3 = 0.0f, t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;
    const float* M = hc->camRot;
    const float O0 = hc->origin[0], O1 = hc->origin[1], O2 = hc->origin[2], ss = hc->screenSize, fl = hc->focalLength, hr = hc->screenHratio;
    FrameConst fc;
    fc.mouse[0] = cam.mouseX; fc.mouse[1] = cam.mouseY; fc.resolution = cam.resolution;
    if (in && !inMouseOverlay(fc, x, y)) {                                                 // 1
        const float4 n0 = rn[4 * p], n1 = rn[4 * p + 1], n2 = rn[4 * p + 2];
        const bool hit = __float_as_int(n1.w) != -1;                                       // 2
        const int mat = __float_as_int(n2.w);
        bool ok;
        float vx, vy, vz;
        if (hit) {
            ok = __builtin_isfinite(n0.x) && finite3(n0.y, n0.z, n0.w) && finite3(n2.x, n2.y, n2.z) && (unsigned)mat < (unsigned)nMat &&
                 (r.allMaterials || !matVD[mat]);
            vx = (cam.On[0] + n0.x * n2.x) - O0; vy = (cam.On[1] + n0.x * n2.y) - O1; vz = (cam.On[2] + n0.x * n2.z) - O2;
        } else {
            ok = true;
            vx = n2.x; vy = n2.y; vz = n2.z;
        }
        const float q0 = (vx * M[0] + vy * M[1]) + vz * M[2];                                  // 3
        const float q1 = (vx * M[3] + vy * M[4]) + vz * M[5];
        const float q2 = (vx * M[6] + vy * M[7]) + vz * M[8];
        const float a = (q0 / q2) * fl, b = (q1 / q2) * fl;                                   // 4
        const float sx = ((1.0f - a / ss) * 0.5f) * (float)W, sy = ((1.0f + b / (hr * ss)) * 0.5f) * (float)H;
        ok = ok && q2 > 0.0f && sx >= 0.0f && sx < (float)W && sy >= 0.0f && sy < (float)H;
        if (ok) {
            const size_t s = (size_t)(int)sy * W + (int)sx;
            const float4 h0 = rh[4 * s], h1 = rh[4 * s + 1], h2 = rh[4 * s + 2];
            const bool hhit = __float_as_int(h1.w) != -1;                                  // 5
            if (hit) {
                const float len = sqrtf((vx * vx + vy * vy) + vz * vz);
                ok = hhit && __float_as_int(h2.w) == mat && __builtin_isfinite(h0.x) && h0.x > 0.0f && __builtin_fabsf(len - h0.x) <= r.depthTol * h0.x &&
                     (n0.y * h0.y + n0.z * h0.z) + n0.w * h0.w >= r.normalTol;
            } else {
                ok = !hhit;
            }
            if (ok) {
                const float4 F = frame[s];                                                 // 6
                ok = F.w > 0.0f && finite3(F.x, F.y, F.z);
                if (ok) {                                                                  // 7
                    const float3 bn = carriedAlbedo(n1, floorA), bh = carriedAlbedo(h1, floorA);
                    f0 = F.x * (bn.x / bh.x); f1 = F.y * (bn.y / bh.y); f2 = F.z * (bn.z / bh.z); f3 = F.w;
                    if (F.w > r.maxHistory) { const float f = r.maxHistory / F.w; f0 = f0 * f; f1 = f1 * f; f2 = f2 * f; f3 = r.maxHistory; }
                    if (stats) {
                        const float rho = lum(bn.x, bn.y, bn.z) / lum(bh.x, bh.y, bh.z);
                        const float4 T = stats[s];
                        t0 = T.x * rho; t1 = (T.y * rho) * rho; t2 = T.z; t3 = T.w;
                        if (T.z > r.maxHistory) { const float g = r.maxHistory / T.z; t0 = t0 * g; t1 = t1 * g; t2 = r.maxHistory; }
                    }
                }
            }
        }
        keep = ok;
    }
    if (in) {
        outFrame[p] = keep ? make_float4(f0, f1, f2, f3) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (outStats) outStats[p] = keep ? make_float4(t0, t1, t2, t3) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const unsigned long long m = __ballot(keep);                                           // every lane of the block, in range or not
    if (threadIdx.x == 0 && m) atomicAdd(&blockKept, (unsigned)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0 && blockKept) atomicAdd(kept, blockKept);
}

}  // namespace

// rn, rh: W*H*4 float4 feature records (include/pt_denoise.h) under the current inputs / the image's camera; frame, stats: the image's FRAME and
// T (stats may be null), W*H float4 in pixel order; hist: the frame constants k_frame_setup built from the image's camera; matVD: nMat bytes,
// 1 = view-dependent material.  cur = (ORIGIN[3], MOUSE_POS.x, MOUSE_POS.y, resolution) of the current inputs, rule = (max_history, depth_tol,
// normal_tol).  Writes outFrame (and outStats when stats is given) and the kept count into *kept.  Enqueued on `s`.
hipError_t reprojectLaunch(const float4* rn, const float4* rh, const float4* frame, const float4* stats, const FrameConst* hist, const unsigned char* matVD,
                           int nMat, int W, int H, const float cur[6], const float rule[3], int allMaterials, float4* outFrame, float4* outStats,
                           unsigned* kept, hipStream_t s) {
    const ReprojCam c{{cur[0], cur[1], cur[2]}, cur[3], cur[4], cur[5]};
    const ReprojRule r{rule[0], rule[1], rule[2], allMaterials};
    hipError_t e = hipMemsetAsync(kept, 0, 4, s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((W + RP_BX - 1) / RP_BX), (unsigned)((H + RP_BY - 1) / RP_BY));
    hipLaunchKernelGGL(k_reproject, grid, dim3(RP_BX, RP_BY), 0, s, rn, rh, frame, stats, hist, matVD, nMat, W, H, c, r, outFrame, outStats, kept);
    return hipGetLastError();
}

// include/pt_demod.h's reprojection: reprojectLaunch with k_reproject_demod.  floorA = albedo_floor, checked by the caller.
hipError_t reprojectDemodLaunch(const float4* rn, const float4* rh, const float4* frame, const float4* stats, const FrameConst* hist, const unsigned char* matVD,
                                int nMat, int W, int H, const float cur[6], const float rule[3], int allMaterials, float floorA, float4* outFrame,
                                float4* outStats, unsigned* kept, hipStream_t s) {
    const ReprojCam c{{cur[0], cur[1], cur[2]}, cur[3], cur[4], cur[5]};
    const ReprojRule r{rule[0], rule[1], rule[2], allMaterials};
    hipError_t e = hipMemsetAsync(kept, 0, 4, s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((W + RP_BX - 1) / RP_BX), (unsigned)((H + RP_BY - 1) / RP_BY));
    hipLaunchKernelGGL(k_reproject_demod, grid, dim3(RP_BX, RP_BY), 0, s, rn, rh, frame, stats, hist, matVD, nMat, W, H, c, r, floorA, outFrame, outStats, kept);
    return hipGetLastError();
}
