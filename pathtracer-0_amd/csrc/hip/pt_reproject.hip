// pt_reproject.hip — the reprojection of include/pt_reproject.h, include/pt_reproject_through.h, include/pt_reproject_bilinear.h and
// include/pt_motion_bilinear.h and the history validation of include/pt_validate.h for gfx950.
//
// Device pointers only: pt_hip.hip owns the buffers, computes both sets of feature records and calls reprojectLaunch on its stream.
//   k_reproject<MOVED, DEMOD, BILINEAR>  one text for the camera and the moved reprojections, from the nearest old pixel and from four taps: each of
//                the steps these share (overlay, Rn[p], the usable hit, the follow-back, the projection, step 7 from one old pixel, the taps and
//                their blend, the kept count) stands once, and the eight instantiations that reprojectLaunch selects are the code objects that
//                three kernel texts with their own copies of these steps were (profiles/r28_reproject_one_text.txt; scripts/kernel_text_diff.py
//                makes the comparison).  One lane per new pixel, a wave = 64 pixels of a row, a block = 16 rows.  Reads 48 B of Rn[p] (F0, F1.w, F2);
//                writes the new pixel of FRAME and T into scratch images.  The kept pixels are counted with a ballot popcount per
//                wave, summed in LDS, and one global atomic per block (one per wave, 32400 on one address at 1080p, cost 0.36 ms).
//                <false, false, false>  include/pt_reproject.h: the same 48 B of Rh[s] at the source pixel (a near-identity gather for small
//                                       moves: the rows of a wave stay together), then FRAME[s] and T[s]
//                <false, true, *>       include/pt_demod.h: step 7 carries illumination
//                <true, *, *>           include/pt_motion.h: the hit's surface point followed back to where its primitive was at the mark (P', N~
//                                       from the mark's and the current positions); the motion loads decide the old pixels' addresses and so precede them
//                <*, *, true>           include/pt_reproject_bilinear.h, include/pt_motion_bilinear.h: each lane blends up to four old pixels around the
//                                       projected point (4 x (24 or 36 B of Rh, FRAME, T), all loaded before the first test) and counts the blended pixels too
//   k_history_merge<R>  include/pt_validate.h: one lane per pixel in the same blocks.  The block's tile with its halo of R pixels is staged in LDS
//                once, as ten planes of floats (the six moments, zeroed where a pixel can be no tap for any centre; the normal; one class /
//                material word), so that a tap costs ten LDS reads of consecutive words per wave and no global load; then steps 1-4 and the
//                reduced count, counted as k_reproject counts the kept pixels.
//   k_through_pack, k_reproject_chain  include/pt_reproject_through.h: behind k_reproject<false, false, false>, the pixels with a seen-through chain take the
//                history of the old pixel whose chain ended on the same surface point, found in a window around the projected virtual point.
// Under the bit-exact contract: binary32 * + / sqrt in the header's order, no contraction (the build's -ffp-contract=off, IEEE divides).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_device.hpp"
#include "pt_image_launch.hpp"

using namespace ptd;

namespace {

constexpr int RP_BX = 64, RP_BY = 16;

__device__ __forceinline__ bool finite3(float a, float b, float c) { return __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c); }
// include/pt_demod.h: b of the header, the floored Kd of a record that is a hit (code != -1) with a finite Kd, else (1, 1, 1).  Kd is F1.xyz of the
// 64-B record whose hit code (F1.w) every kernel reads: the demodulated and the moved kernels load the 16 B, the plain one the 4 B of the code.
__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ float3 carriedAlbedo(const float4 f1, float floorA) {
    return __float_as_int(f1.w) != -1 && finite3(f1.x, f1.y, f1.z) ? make_float3(fmaxf(f1.x, floorA), fmaxf(f1.y, floorA), fmaxf(f1.z, floorA))
                                                                  : make_float3(1.0f, 1.0f, 1.0f);
}
__device__ __forceinline__ float dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
// F1 of a 64-B record: all of it (the Kd that step 7 carries; the moved kernels' one load), or the 4 B of its hit code alone, in the w
template <bool WHOLE>
__device__ __forceinline__ float4 loadF1(const float4* __restrict__ rec) {
    if constexpr (WHOLE) return rec[1];
    else return make_float4(0.0f, 0.0f, 0.0f, reinterpret_cast<const float*>(rec + 1)[3]);
}
// Own: the arguments a specialisation has of its own, so that each keeps its kernarg layout — nearest: none, (floorA) when DEMOD, (g, floorA) when
// MOVED; bilinear: (snap, floorA), then g when MOVED
__device__ __forceinline__ const ReprojMotion& motionOf(const ReprojMotion& g, float) { return g; }
__device__ __forceinline__ const ReprojMotion& motionOf(float, float, const ReprojMotion& g) { return g; }
__device__ __forceinline__ float floorOf(float floorA) { return floorA; }
__device__ __forceinline__ float floorOf(const ReprojMotion&, float floorA) { return floorA; }
template <class... G>
__device__ __forceinline__ float floorOf(float, float floorA, const G&...) { return floorA; }
template <class... G>
__device__ __forceinline__ float snapOf(float snap, float, const G&...) { return snap; }

// Steps 3-4 of include/pt_reproject.h: v = P - O taken into the image's camera M and projected to the pixel coordinates (sx, sy); on: in front of the
// camera and inside the image
struct ImagePoint { float sx, sy; bool on; };
__device__ __forceinline__ ImagePoint projectToImage(float vx, float vy, float vz, const float* __restrict__ M, float ss, float fl, float hr, int W, int H) {
    const float q0 = (vx * M[0] + vy * M[1]) + vz * M[2];                                      // 3
    const float q1 = (vx * M[3] + vy * M[4]) + vz * M[5];
    const float q2 = (vx * M[6] + vy * M[7]) + vz * M[8];
    const float a = (q0 / q2) * fl, b = (q1 / q2) * fl;                                       // 4
    const float sx = ((1.0f - a / ss) * 0.5f) * (float)W, sy = ((1.0f + b / (hr * ss)) * 0.5f) * (float)H;
    return {sx, sy, q2 > 0.0f && sx >= 0.0f && sx < (float)W && sy >= 0.0f && sy < (float)H};
}

// Step 7 of include/pt_reproject.h from one old pixel: its FRAME F and, where hasT says that the context has T, its T from loadT(), both capped at
// maxHistory.  DEMOD: F scaled by bn / bh and T by rho = l(bn) / l(bh) before the caps (include/pt_demod.h), bn and bh the carried albedos of the
// new and the old pixel.  The results are reference parameters and the cap multiplies named temporaries: this is the form that compiles to the
// instruction streams the kernels had when each held this text itself.
template <bool DEMOD, class HasT, class LoadT>
__device__ __forceinline__ void carryOne(float maxHistory, const float4 F, const float3 bn, const float3 bh, HasT hasT, LoadT loadT, float& f0, float& f1, float& f2,
                                         float& f3, float& t0, float& t1, float& t2, float& t3) {
    if constexpr (DEMOD) {
        f0 = F.x * (bn.x / bh.x); f1 = F.y * (bn.y / bh.y); f2 = F.z * (bn.z / bh.z); f3 = F.w;
        if (F.w > maxHistory) { const float f = maxHistory / F.w; f0 = f0 * f; f1 = f1 * f; f2 = f2 * f; f3 = maxHistory; }
        if (hasT) {
            const float rho = lum(bn.x, bn.y, bn.z) / lum(bh.x, bh.y, bh.z);
            const float4 T = loadT();
            const float y = T.x * rho, yy = (T.y * rho) * rho;
            t0 = y; t1 = yy; t2 = T.z; t3 = T.w;
            if (T.z > maxHistory) { const float gg = maxHistory / T.z; t0 = y * gg; t1 = yy * gg; t2 = maxHistory; }
        }
    } else {
        f0 = F.x; f1 = F.y; f2 = F.z; f3 = F.w;
        if (F.w > maxHistory) { const float f = maxHistory / F.w; f0 = F.x * f; f1 = F.y * f; f2 = F.z * f; f3 = maxHistory; }
        if (hasT) {
            const float4 T = loadT();
            t0 = T.x; t1 = T.y; t2 = T.z; t3 = T.w;
            if (T.z > maxHistory) { const float gg = maxHistory / T.z; t0 = T.x * gg; t1 = T.y * gg; t2 = maxHistory; }
        }
    }
}

// include/pt_reproject_bilinear.h, step 5 along one axis: the first tap's coordinate (-1 .. size - 1) and the second tap's weight after snapping
__device__ __forceinline__ int bilinearAxis(float s, float snap, float& w) {
    const float f = s - 0.5f;
    float c0 = floorf(f);
    w = f - c0;
    if (w < snap) w = 0.0f;
    else if (w > 1.0f - snap) { c0 = c0 + 1.0f; w = 0.0f; }
    return (int)c0;
}
// One tap of include/pt_reproject_bilinear.h: what the lane loaded of old pixel s (clamped into the image, so every load is in range) and its weight.
// Of Rh[s]: h0 = F0 (t', N'), h1 = all of F1 when DEMOD, else the hit code in its w, mat = the material word of F2 — what step 5 and the carried albedo read.
struct BilinearTap { float4 h0, h1, F, T; int mat; float w; bool in; };

// The camera and the moved reprojections, from the nearest old pixel and from four taps: one text, eight instantiations.
//   steps 1-4 of include/pt_reproject.h: overlay, Rn[p], the usable hit, the projection into the image's camera.
//   MOVED: step 2 follows the hit's surface point back to where its primitive was at the mark (P', N~), and the old pixels are tested against |v| of
//   P' and against N~ (include/pt_motion.h).  A lane on an unmoved primitive pays one 16-B load (the record that holds the flag); a moved triangle
//   96 B, a moved ellipsoid 64 B.  These loads decide sx and sy, so they precede every load of an old pixel.
//   !BILINEAR: steps 5-7 of include/pt_reproject.h from the pixel s that holds (sx, sy): 48 B of Rh[s], FRAME[s], T[s].
//   BILINEAR: steps 5-9 of include/pt_reproject_bilinear.h (and of include/pt_motion_bilinear.h).  Of each of the four taps the 24 B of Rh[s] that
//   step 5 reads (36 B with DEMOD: Kd too), FRAME (16 B) and T (16 B), loaded from clamped addresses before the first test and without a branch
//   between them, so that the twenty loads are in flight together; the two x-taps of a row are adjacent 64-B records.  (Loading all 48 B of F0 .. F2
//   made the compiler reuse the registers of the unread D' while the load was in flight, with a wait in front of every tap.)  A context without T
//   reads FRAME in T's place and ignores it.  The taps and the accumulators are scalars (four named structs, no indexed array): nothing on the stack.
//   Step 7 from one old pixel (carryOne) serves the nearest pixel and the one tap that counts.
//   kept[0] takes the kept pixels and, BILINEAR, kept[1] those blended from two or more taps: a ballot popcount per wave, an LDS sum, one atomic per
//   block and counter.
template <bool MOVED, bool DEMOD, bool BILINEAR, class... Own>
__global__ void __launch_bounds__(RP_BX * RP_BY) k_reproject(const float4* __restrict__ rn, const float4* __restrict__ rh, const float4* __restrict__ frame,
                                                            const float4* __restrict__ stats, const FrameConst* __restrict__ hc, const unsigned char* __restrict__ matVD,
                                                            int nMat, int W, int H, ReprojCam cam, ReprojRule r, Own... own,
                                                            float4* __restrict__ outFrame, float4* __restrict__ outStats, unsigned* __restrict__ kept) {
    __shared__ unsigned blockKept, blockBlended;
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        blockKept = 0;
        if constexpr (BILINEAR) blockBlended = 0;
    }
    __syncthreads();
    const int x = blockIdx.x * RP_BX + threadIdx.x, y = blockIdx.y * RP_BY + threadIdx.y;
    const bool in = x < W && y < H;
    const size_t p = (size_t)y * W + x;
    bool keep = false, blended = false;
    float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f, f3 = 0.0f, t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;      // the new FRAME and T (scalars: no stack copy)
    const float* M = hc->camRot;                                                           // the image's camera, as k_frame_setup built it
    const float O0 = hc->origin[0], O1 = hc->origin[1], O2 = hc->origin[2], ss = hc->screenSize, fl = hc->focalLength, hr = hc->screenHratio;
    FrameConst fc;
    fc.mouse[0] = cam.mouseX; fc.mouse[1] = cam.mouseY; fc.resolution = cam.resolution;
    if (in && !inMouseOverlay(fc, x, y)) {                                                 // 1
        constexpr bool WHOLE_F1 = BILINEAR ? DEMOD : MOVED || DEMOD;                       // the nearest moved kernels' one load of the record
        const float4 n0 = rn[4 * p], n2 = rn[4 * p + 2];
        const float4 n1 = loadF1<WHOLE_F1>(rn + 4 * p);
        const int code = __float_as_int(n1.w);
        const bool hit = code != -1;                                                       // 2
        const int mat = __float_as_int(n2.w);
        bool ok;
        float vx, vy, vz;
        float Nx = n0.y, Ny = n0.z, Nz = n0.w;                                             // N~: the normal the surface point had at the mark
        if (hit) {
            ok = __builtin_isfinite(n0.x) && finite3(n0.y, n0.z, n0.w) && finite3(n2.x, n2.y, n2.z) && (unsigned)mat < (unsigned)nMat &&
                 (r.allMaterials || !matVD[mat]);
            if constexpr (MOVED) {
                float Px = cam.On[0] + n0.x * n2.x, Py = cam.On[1] + n0.x * n2.y, Pz = cam.On[2] + n0.x * n2.z;      // P, then P'
                const ReprojMotion& g = motionOf(own...);
                const unsigned type = (unsigned)code >> 24;
                const int id = code & 0xffffff;
                if (!ok) {
                } else if (type == 1u) {
                    if (id < g.nTriNow && id < g.nTriThen) {
                        const float4 A = g.triNow[3 * (size_t)id];
                        if (__float_as_int(A.w) != 0) {                                        // moved: through the barycentrics of P in (A, B, C)
                            const float4 B = g.triNow[3 * (size_t)id + 1], C = g.triNow[3 * (size_t)id + 2];
                            const float4 Ah = g.triThen[3 * (size_t)id], Bh = g.triThen[3 * (size_t)id + 1], Ch = g.triThen[3 * (size_t)id + 2];
                            const float e1x = B.x - A.x, e1y = B.y - A.y, e1z = B.z - A.z, e2x = C.x - A.x, e2y = C.y - A.y, e2z = C.z - A.z;
                            const float wx = Px - A.x, wy = Py - A.y, wz = Pz - A.z;
                            const float h1x = Bh.x - Ah.x, h1y = Bh.y - Ah.y, h1z = Bh.z - Ah.z, h2x = Ch.x - Ah.x, h2y = Ch.y - Ah.y, h2z = Ch.z - Ah.z;
                            const float d11 = dot3(e1x, e1y, e1z, e1x, e1y, e1z), d12 = dot3(e1x, e1y, e1z, e2x, e2y, e2z), d22 = dot3(e2x, e2y, e2z, e2x, e2y, e2z);
                            const float den = d11 * d22 - d12 * d12;
                            const float w1 = dot3(wx, wy, wz, e1x, e1y, e1z), w2 = dot3(wx, wy, wz, e2x, e2y, e2z);
                            const float beta = (d22 * w1 - d12 * w2) / den, gamma = (d11 * w2 - d12 * w1) / den;
                            Px = (Ah.x + beta * h1x) + gamma * h2x; Py = (Ah.y + beta * h1y) + gamma * h2y; Pz = (Ah.z + beta * h1z) + gamma * h2z;
                            const float gx = e1y * e2z - e1z * e2y, gy = e1z * e2x - e1x * e2z, gz = e1x * e2y - e1y * e2x;
                            const float kx = h1y * h2z - h1z * h2y, ky = h1z * h2x - h1x * h2z, kz = h1x * h2y - h1y * h2x;
                            const float m1 = dot3(Nx, Ny, Nz, e1x, e1y, e1z), m2 = dot3(Nx, Ny, Nz, e2x, e2y, e2z);
                            const float a = (d22 * m1 - d12 * m2) / den, b = (d11 * m2 - d12 * m1) / den;
                            const float c = dot3(Nx, Ny, Nz, gx, gy, gz) / dot3(gx, gy, gz, gx, gy, gz);
                            const float Mx = (a * h1x + b * h2x) + c * kx, My = (a * h1y + b * h2y) + c * ky, Mz = (a * h1z + b * h2z) + c * kz;
                            const float ml = sqrtf(dot3(Mx, My, Mz, Mx, My, Mz));
                            Nx = Mx / ml; Ny = My / ml; Nz = Mz / ml;
                            ok = __builtin_isfinite(den) && den > 0.0f && finite3(Px, Py, Pz) && finite3(Nx, Ny, Nz);
                        }
                    } else {
                        ok = false;
                    }
                } else if (type == 3u) {
                    if (id < g.nElNow && id < g.nElThen) {
                        const float4 S = g.elNow[3 * (size_t)id + 1];
                        const int flag = __float_as_int(S.w);
                        if (flag == 1) {                                                       // moved, no rotation: the point keeps its place on the unit sphere
                            const float4 Cn = g.elNow[3 * (size_t)id], Ch = g.elThen[3 * (size_t)id], Sh = g.elThen[3 * (size_t)id + 1];
                            const float rr = Ch.w / Cn.w;
                            const float k0 = sqrtf(S.x / Sh.x) * rr, k1 = sqrtf(S.y / Sh.y) * rr, k2 = sqrtf(S.z / Sh.z) * rr;
                            Px = Ch.x + (Px - Cn.x) * k0; Py = Ch.y + (Py - Cn.y) * k1; Pz = Ch.z + (Pz - Cn.z) * k2;
                            ok = finite3(Px, Py, Pz);
                        } else if (flag != 0) {
                            ok = false;
                        }
                    } else {
                        ok = false;
                    }
                } else {
                    ok = false;
                }
                vx = Px - O0; vy = Py - O1; vz = Pz - O2;
            } else {                                                                       // P - O, a component at a time (the compiler pairs them into packed operations by this order)
                vx = (cam.On[0] + n0.x * n2.x) - O0; vy = (cam.On[1] + n0.x * n2.y) - O1; vz = (cam.On[2] + n0.x * n2.z) - O2;
            }
        } else {
            ok = true;
            vx = n2.x; vy = n2.y; vz = n2.z;
        }
        const ImagePoint at = projectToImage(vx, vy, vz, M, ss, fl, hr, W, H);                // 3, 4
        const float sx = at.sx, sy = at.sy;
        ok = ok && at.on;
        if (ok) {
            auto albedo = [&](const float4 f1) {                                           // b of include/pt_demod.h; (1, 1, 1) where nothing is demodulated
                if constexpr (DEMOD) return carriedAlbedo(f1, floorOf(own...));
                else return make_float3(1.0f, 1.0f, 1.0f);
            };
            if constexpr (BILINEAR) {
                float wx, wy;                                                              // 5
                const float snap = snapOf(own...);
                const int ix = bilinearAxis(sx, snap, wx), iy = bilinearAxis(sy, snap, wy);
                const float ax0 = 1.0f - wx, ay0 = 1.0f - wy;
                const int cx0 = min(max(ix, 0), W - 1), cx1 = min(max(ix + 1, 0), W - 1), cy0 = min(max(iy, 0), H - 1), cy1 = min(max(iy + 1, 0), H - 1);
                const bool inx0 = ix >= 0 && ix < W, inx1 = ix + 1 < W, iny0 = iy >= 0 && iy < H, iny1 = iy + 1 < H;      // (ix, iy >= -1)
                const bool hasT = stats != nullptr;
                const float4* __restrict__ tsrc = hasT ? stats : frame;
                auto load = [&](int cx, int cy, float w, bool inside) {
                    const size_t s = (size_t)cy * W + cx;
                    BilinearTap t;
                    t.h0 = rh[4 * s]; t.h1 = loadF1<WHOLE_F1>(rh + 4 * s); t.mat = __float_as_int(reinterpret_cast<const float*>(rh + 4 * s)[11]);
                    t.F = frame[s];
                    t.T = tsrc[s];
                    t.w = w; t.in = inside;
                    return t;
                };
                const BilinearTap ta = load(cx0, cy0, ax0 * ay0, inx0 && iny0), tb = load(cx1, cy0, wx * ay0, inx1 && iny0);
                const BilinearTap tc = load(cx0, cy1, ax0 * wy, inx0 && iny1), td = load(cx1, cy1, wx * wy, inx1 && iny1);
                const float len = sqrtf((vx * vx + vy * vy) + vz * vz);
                auto counts = [&](const BilinearTap& t) {
                    const bool hhit = __float_as_int(t.h1.w) != -1;
                    const bool same = hit ? hhit && t.mat == mat && __builtin_isfinite(t.h0.x) && t.h0.x > 0.0f &&
                                                __builtin_fabsf(len - t.h0.x) <= r.depthTol * t.h0.x && (Nx * t.h0.y + Ny * t.h0.z) + Nz * t.h0.w >= r.normalTol
                                          : !hhit;
                    return t.w > 0.0f && t.in && same && t.F.w > 0.0f && finite3(t.F.x, t.F.y, t.F.z);
                };
                const bool ca = counts(ta), cb = counts(tb), cc = counts(tc), cd = counts(td);
                const int nc = (int)ca + (int)cb + (int)cc + (int)cd;
                const float3 bn = albedo(n1);
                if (nc == 1) {                                                             // 7: from the one tap
                    const float4 F = ca ? ta.F : cb ? tb.F : cc ? tc.F : td.F, T = ca ? ta.T : cb ? tb.T : cc ? tc.T : td.T;
                    carryOne<DEMOD>(r.maxHistory, F, bn, albedo(ca ? ta.h1 : cb ? tb.h1 : cc ? tc.h1 : td.h1), hasT, [T] { return T; }, f0, f1, f2, f3, t0, t1, t2, t3);
                } else if (nc >= 2) {                                                      // 8, 9: a tap that does not count adds +0, which changes no bit of a sum that began at +0
                    float Ws = 0.0f, A = 0.0f, C0 = 0.0f, C1 = 0.0f, C2 = 0.0f, WT = 0.0f, NT = 0.0f, Y = 0.0f, YY = 0.0f;
                    auto add = [&](const BilinearTap& t, bool c) {
                        float m0 = t.F.x / t.F.w, m1 = t.F.y / t.F.w, m2 = t.F.z / t.F.w;
                        float rho = 1.0f;
                        if constexpr (DEMOD) {
                            const float3 bh = albedo(t.h1);
                            m0 = m0 * (bn.x / bh.x); m1 = m1 * (bn.y / bh.y); m2 = m2 * (bn.z / bh.z);
                            rho = lum(bn.x, bn.y, bn.z) / lum(bh.x, bh.y, bh.z);
                        }
                        Ws = Ws + (c ? t.w : 0.0f); A = A + (c ? t.w * t.F.w : 0.0f);
                        C0 = C0 + (c ? t.w * m0 : 0.0f); C1 = C1 + (c ? t.w * m1 : 0.0f); C2 = C2 + (c ? t.w * m2 : 0.0f);
                        const bool ct = hasT && c && t.T.z > 0.0f && __builtin_isfinite(t.T.x) && __builtin_isfinite(t.T.y);
                        float yv = t.T.x / t.T.z, yy = t.T.y / t.T.z;
                        if constexpr (DEMOD) { yv = yv * rho; yy = (yy * rho) * rho; }
                        WT = WT + (ct ? t.w : 0.0f); NT = NT + (ct ? t.w * t.T.z : 0.0f); Y = Y + (ct ? t.w * yv : 0.0f); YY = YY + (ct ? t.w * yy : 0.0f);
                    };
                    add(ta, ca); add(tb, cb); add(tc, cc); add(td, cd);
                    const float n = A / Ws, nn = n > r.maxHistory ? r.maxHistory : n;
                    f0 = (C0 / Ws) * nn; f1 = (C1 / Ws) * nn; f2 = (C2 / Ws) * nn; f3 = nn;
                    if (WT > 0.0f) {
                        const float nT = NT / WT, nt = nT > r.maxHistory ? r.maxHistory : nT;
                        t0 = (Y / WT) * nt; t1 = (YY / WT) * nt; t2 = nt; t3 = 0.0f;
                    }
                    blended = true;
                }
                ok = nc >= 1;                                                              // 6
            } else {
                const size_t s = (size_t)(int)sy * W + (int)sx;
                const float4 h0 = rh[4 * s], h2 = rh[4 * s + 2];
                const float4 h1 = loadF1<WHOLE_F1>(rh + 4 * s);
                const bool hhit = __float_as_int(h1.w) != -1;                              // 5
                if (hit) {
                    const float len = sqrtf((vx * vx + vy * vy) + vz * vz);
                    ok = hhit && __float_as_int(h2.w) == mat && __builtin_isfinite(h0.x) && h0.x > 0.0f && __builtin_fabsf(len - h0.x) <= r.depthTol * h0.x &&
                         (Nx * h0.y + Ny * h0.z) + Nz * h0.w >= r.normalTol;
                } else {
                    ok = !hhit;
                }
                if (ok) {
                    const float4 F = frame[s];                                             // 6
                    ok = F.w > 0.0f && finite3(F.x, F.y, F.z);
                    if (ok) carryOne<DEMOD>(r.maxHistory, F, albedo(n1), albedo(h1), stats, [&] { return stats[s]; }, f0, f1, f2, f3, t0, t1, t2, t3);                     // 7
                }
            }
        }
        keep = ok;
    }
    if (in) {
        outFrame[p] = keep ? make_float4(f0, f1, f2, f3) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (outStats) outStats[p] = keep ? make_float4(t0, t1, t2, t3) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const unsigned long long m = __ballot(keep), mb = __ballot(blended);                   // every lane of the block, in range or not
    if (threadIdx.x == 0 && m) atomicAdd(&blockKept, (unsigned)__popcll(m));
    if constexpr (BILINEAR) if (threadIdx.x == 0 && mb) atomicAdd(&blockBlended, (unsigned)__popcll(mb));
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        if (blockKept) atomicAdd(kept, blockKept);
        if constexpr (BILINEAR) if (blockBlended) atomicAdd(kept + 1, blockBlended);
    }
}

// max(x, 0) of include/pt_guided.h: a NaN is no estimate
__device__ __forceinline__ float clampVar(float x) { return x >= 0.0f ? x : (x < 0.0f ? 0.0f : __builtin_inff()); }

// include/pt_validate.h, steps 1-4.  The tile: pixel (tx, ty) of the block's 64 x 16 plus a halo of R on every side, plane by plane.  A pixel that
// fails what no centre can mend (outside the image, not paired, a sum that is not finite) has its six moments stored as zeros: adding +0 to a sum
// that started at +0 changes no bit of it, so the tap loop needs no test for these.  The word plane holds the material word of a hit and -1 for a
// miss — k_feature_record gives a hit the index of its material, never -1 — so that "p's class and, for a hit, p's material" is one compare.
struct ValidateRule { float zLo, zHi, normalTol, mouseX, mouseY, resolution; };
template <int R>
__global__ void __launch_bounds__(RP_BX * RP_BY) k_history_merge(const float4* __restrict__ rec, const float4* __restrict__ frameN, const float4* __restrict__ statsU,
                                                                const float4* __restrict__ frameH, const float4* __restrict__ statsV, int W, int H, ValidateRule r,
                                                                float4* __restrict__ outFrame, float4* __restrict__ outStats, float* __restrict__ kappaOut,
                                                                unsigned* __restrict__ reduced) {
    constexpr int TW = RP_BX + 2 * R, TH = RP_BY + 2 * R, TN = TW * TH;
    enum { SY_N, SYY_N, N_N, SY_H, SYY_H, N_H, NX, NY, NZ, WORD, PLANES };
    __shared__ float tile[PLANES][TN];
    __shared__ unsigned blockReduced;
    const int tid = threadIdx.y * RP_BX + threadIdx.x;
    if (tid == 0) blockReduced = 0;
    const int x0 = blockIdx.x * RP_BX - R, y0 = blockIdx.y * RP_BY - R;
    for (int i = tid; i < TN; i += RP_BX * RP_BY) {
        const int gx = x0 + i % TW, gy = y0 + i / TW;
        float4 U = make_float4(0.0f, 0.0f, 0.0f, 0.0f), V = U, f0 = U;
        int word = -1;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gy * W + gx;
            const float4 u = statsU[g], v = statsV[g];
            if (u.z >= 1.0f && v.z >= 1.0f && __builtin_isfinite(u.x) && __builtin_isfinite(u.y) && __builtin_isfinite(v.x) && __builtin_isfinite(v.y)) { U = u; V = v; }
            f0 = rec[4 * g];
            const float* w = reinterpret_cast<const float*>(rec + 4 * g);
            word = __float_as_int(w[7]) != -1 ? __float_as_int(w[11]) : -1;
        }
        tile[SY_N][i] = U.x; tile[SYY_N][i] = U.y; tile[N_N][i] = U.z; tile[SY_H][i] = V.x; tile[SYY_H][i] = V.y; tile[N_H][i] = V.z;
        tile[NX][i] = f0.y; tile[NY][i] = f0.z; tile[NZ][i] = f0.w; tile[WORD][i] = __int_as_float(word);
    }
    __syncthreads();
    const int x = blockIdx.x * RP_BX + threadIdx.x, y = blockIdx.y * RP_BY + threadIdx.y;
    const bool in = x < W && y < H;
    bool less = false;
    if (in) {
        float kappa = 1.0f;
        FrameConst fc;
        fc.mouse[0] = r.mouseX; fc.mouse[1] = r.mouseY; fc.resolution = r.resolution;
        if (!inMouseOverlay(fc, x, y)) {                                                   // 1
            const int c = (threadIdx.y + R) * TW + threadIdx.x + R;
            const float Nx = tile[NX][c], Ny = tile[NY][c], Nz = tile[NZ][c];
            const int word = __float_as_int(tile[WORD][c]);
            float SN = 0.0f, QN = 0.0f, NN = 0.0f, SH = 0.0f, QH = 0.0f, NH = 0.0f;
#pragma unroll 1
            for (int dy = -R; dy <= R; dy++) {                                             // 2: a row of taps at a time in registers (all of them spill)
#pragma unroll
                for (int dx = -R; dx <= R; dx++) {
                    const int q = c + dy * TW + dx;
                    const bool tap = __float_as_int(tile[WORD][q]) == word && (word == -1 || dot3(Nx, Ny, Nz, tile[NX][q], tile[NY][q], tile[NZ][q]) >= r.normalTol);
                    SN = SN + (tap ? tile[SY_N][q] : 0.0f); QN = QN + (tap ? tile[SYY_N][q] : 0.0f); NN = NN + (tap ? tile[N_N][q] : 0.0f);
                    SH = SH + (tap ? tile[SY_H][q] : 0.0f); QH = QH + (tap ? tile[SYY_H][q] : 0.0f); NH = NH + (tap ? tile[N_H][q] : 0.0f);
                }
            }
            if (NN >= 2.0f && NH >= 2.0f) {                                                // 3
                const float mN = SN / NN, s2N = clampVar((QN - SN * mN) / (NN - 1.0f));
                const float mH = SH / NH, s2H = clampVar((QH - SH * mH) / (NH - 1.0f));
                const float var = s2N / NN + s2H / NH;
                const float d = __builtin_fabsf(mN - mH);
                const float z = sqrtf((d * d) / var);
                if (z != z || z <= r.zLo) kappa = 1.0f;
                else if (z >= r.zHi) kappa = 0.0f;
                else kappa = (r.zHi - z) / (r.zHi - r.zLo);
            }
        }
        const size_t p = (size_t)y * W + x;                                                // 4
        const float4 N = frameN[p], U = statsU[p], Hh = frameH[p];
        float4 F = N, T = make_float4(U.x, U.y, U.z, 0.0f);
        if (kappa != 0.0f) {
            const float4 V = statsV[p];
            F = make_float4(N.x + kappa * Hh.x, N.y + kappa * Hh.y, N.z + kappa * Hh.z, N.w + kappa * Hh.w);
            T = make_float4(U.x + kappa * V.x, U.y + kappa * V.y, U.z + kappa * V.z, 0.0f);
        }
        outFrame[p] = F; outStats[p] = T;
        if (kappaOut) kappaOut[p] = kappa;
        less = Hh.w > 0.0f && kappa < 1.0f;
    }
    const unsigned long long m = __ballot(less);                                           // every lane of the block, in range or not
    if (threadIdx.x == 0 && m) atomicAdd(&blockReduced, (unsigned)__popcll(m));
    __syncthreads();
    if (tid == 0 && blockReduced) atomicAdd(reduced, blockReduced);
}

// include/pt_reproject_through.h, per pixel s of the image's camera: what a candidate test of step 5 reads, 32 B in place of the 80 B of Sh[s], Yh[s] and
// FRAME[s].  pack[2s] = (X', surface word), pack[2s + 1] = (N', usable as an int: Sh[s] is a hit, X' is finite, FRAME[s].a > 0 with a finite rgb)
constexpr int TP_B = 256;
__global__ void __launch_bounds__(TP_B) k_through_pack(const float4* __restrict__ sh, const float4* __restrict__ yh, const float4* __restrict__ frame, int n,
                                                      float4* __restrict__ pack) {
    const int s = blockIdx.x * TP_B + threadIdx.x;
    if (s >= n) return;
    const float4 s0 = sh[4 * (size_t)s];
    const float* w = reinterpret_cast<const float*>(sh + 4 * (size_t)s);
    const float4 y0 = yh[2 * (size_t)s], y1 = yh[2 * (size_t)s + 1], F = frame[s];
    const float X0 = y0.x + y0.w * y1.x, X1 = y0.y + y0.w * y1.y, X2 = y0.z + y0.w * y1.z;
    const bool usable = __float_as_int(w[7]) != -1 && finite3(X0, X1, X2) && F.w > 0.0f && finite3(F.x, F.y, F.z);
    pack[2 * (size_t)s] = make_float4(X0, X1, X2, w[11]);
    pack[2 * (size_t)s + 1] = make_float4(s0.y, s0.z, s0.w, __int_as_float(usable ? 1 : 0));
}

// Steps 3-6 of include/pt_reproject_through.h, behind k_reproject<false, false, false> on the same stream: that launch has given every pixel steps
// 1-2 (a chain pixel among them the verdict of its first hit, which this kernel replaces), so that the steps the two headers share have one
// definition.  Its step 4 is projectToImage; its step 6 keeps its own plain step 7, which stores FRAME before it loads T (through carryOne the
// kernel came out three instructions longer).  One lane per new pixel in k_reproject's blocks; a lane whose k_p is 0 (4 B read) or that lies
// under the overlay is done.  The window's centre depends on the data, so a block's candidates are no tile: the (2 radius + 1)^2 loop reads the packed
// pixels of k_through_pack straight from L2, 16 B for a candidate of another surface word, 32 B otherwise; neighbouring lanes have neighbouring
// centres.  The loops are not unrolled (radius is an argument; 81 unrolled candidates would not fit in registers).  kept[0] takes kept-now minus
// kept-by-the-first-hit (modulo 2^32), kept[1] the chain pixels kept: k_reproject's scheme, a ballot popcount per wave, an LDS sum, one atomic
// per block and counter.
__global__ void __launch_bounds__(RP_BX * RP_BY) k_reproject_chain(const float4* __restrict__ sn, const float4* __restrict__ yn, const float4* __restrict__ pack,
                                                                  const float4* __restrict__ frame, const float4* __restrict__ stats, const FrameConst* __restrict__ hc,
                                                                  const unsigned char* __restrict__ matVD, int nMat, int W, int H, ReprojCam cam, ReprojRule r,
                                                                  float pointTol, int radius, float4* __restrict__ outFrame, float4* __restrict__ outStats,
                                                                  unsigned* __restrict__ kept) {
    __shared__ unsigned blockKept, blockWas;
    if (threadIdx.x == 0 && threadIdx.y == 0) { blockKept = 0; blockWas = 0; }
    __syncthreads();
    const int x = blockIdx.x * RP_BX + threadIdx.x, y = blockIdx.y * RP_BY + threadIdx.y;
    const bool in = x < W && y < H;
    const size_t p = (size_t)y * W + x;
    bool keep = false, was = false;
    FrameConst fc;
    fc.mouse[0] = cam.mouseX; fc.mouse[1] = cam.mouseY; fc.resolution = cam.resolution;
    if (in && !inMouseOverlay(fc, x, y) && __float_as_int(reinterpret_cast<const float*>(sn + 4 * p)[14]) >= 1) {      // 1, 2
        was = outFrame[p].w > 0.0f;                                                        // a kept pixel has a count > 0
        const float4 s0 = sn[4 * p], s2 = sn[4 * p + 2], y0 = yn[2 * p], y1 = yn[2 * p + 1];
        const int code = __float_as_int(reinterpret_cast<const float*>(sn + 4 * p)[7]), word = __float_as_int(s2.w), mat = word & 0xfff;
        const float L = s0.x;
        bool ok = code != -1 && __builtin_isfinite(L) && L > 0.0f && finite3(s0.y, s0.z, s0.w) && finite3(s2.x, s2.y, s2.z) && finite3(y0.x, y0.y, y0.z) &&
                  __builtin_isfinite(y0.w) && finite3(y1.x, y1.y, y1.z) && mat < nMat && (r.allMaterials || !matVD[mat]);      // 3
        const float X0 = y0.x + y0.w * y1.x, X1 = y0.y + y0.w * y1.y, X2 = y0.z + y0.w * y1.z;
        const float* M = hc->camRot;                                                       // 4: the virtual point in the image's camera
        const float vx = (cam.On[0] + L * s2.x) - hc->origin[0], vy = (cam.On[1] + L * s2.y) - hc->origin[1], vz = (cam.On[2] + L * s2.z) - hc->origin[2];
        const ImagePoint at = projectToImage(vx, vy, vz, M, hc->screenSize, hc->focalLength, hc->screenHratio, W, H);
        const float sx = at.sx, sy = at.sy;
        ok = ok && at.on;
        if (ok) {                                                                          // 5
            const int cx = (int)sx, cy = (int)sy;
            const int xLo = max(cx - radius, 0), xHi = min(cx + radius, W - 1), yLo = max(cy - radius, 0), yHi = min(cy + radius, H - 1);
            const float tol = pointTol * L, tol2 = tol * tol;
            float best = 0.0f;
            long long src = -1;
#pragma unroll 1
            for (int yy = yLo; yy <= yHi; yy++) {
#pragma unroll 1
                for (int xx = xLo; xx <= xHi; xx++) {
                    const size_t s = (size_t)yy * W + xx;
                    const float4 c0 = pack[2 * s];
                    if (__float_as_int(c0.w) != word) continue;
                    const float4 c1 = pack[2 * s + 1];
                    const float e0 = c0.x - X0, e1 = c0.y - X1, e2 = c0.z - X2;
                    const float d2 = (e0 * e0 + e1 * e1) + e2 * e2;
                    if (__float_as_int(c1.w) != 0 && d2 <= tol2 && dot3(s0.y, s0.z, s0.w, c1.x, c1.y, c1.z) >= r.normalTol && (src < 0 || d2 < best)) {
                        best = d2; src = (long long)s;
                    }
                }
            }
            ok = src >= 0;
            if (ok) {                                                                      // 6: step 7 of include/pt_reproject.h
                const float4 F = frame[src];
                float4 o = F, t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (F.w > r.maxHistory) { const float f = r.maxHistory / F.w; o = make_float4(F.x * f, F.y * f, F.z * f, r.maxHistory); }
                outFrame[p] = o;
                if (outStats) {
                    const float4 T = stats[src];
                    t = T;
                    if (T.z > r.maxHistory) { const float gg = r.maxHistory / T.z; t = make_float4(T.x * gg, T.y * gg, r.maxHistory, T.w); }
                    outStats[p] = t;
                }
            }
        }
        if (!ok && was) {                                                                  // kept by its first hit (PT_REPROJECT_ALL_MATERIALS), rejected by its chain
            outFrame[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (outStats) outStats[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        keep = ok;
    }
    const unsigned long long m = __ballot(keep), mw = __ballot(was);                       // every lane of the block, in range or not
    if (threadIdx.x == 0 && m) atomicAdd(&blockKept, (unsigned)__popcll(m));
    if (threadIdx.x == 0 && mw) atomicAdd(&blockWas, (unsigned)__popcll(mw));
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        if (blockKept != blockWas) atomicAdd(kept, blockKept - blockWas);
        if (blockKept) atomicAdd(kept + 1, blockKept);
    }
}

}  // namespace

// floorA > 0 alone selects the demodulated step 7, `motion` alone the followed-back step 2
hipError_t reprojectLaunch(const ReprojectJob& j, hipStream_t s) {
    hipError_t e = hipMemsetAsync(j.kept, 0, j.sn || j.bilinear ? 8 : 4, s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((j.W + RP_BX - 1) / RP_BX), (unsigned)((j.H + RP_BY - 1) / RP_BY)), block(RP_BX, RP_BY);
    if (j.bilinear && j.sn) return hipErrorInvalidValue;                                   // the bilinear mapping is one of its own: no chain pixels on top
    const bool demod = j.floorA > 0.0f;
    auto launch = [&](auto kernel, auto... own) {                                          // own: the instantiation's arguments, where its kernarg layout has them
        hipLaunchKernelGGL(kernel, grid, block, 0, s, j.rn, j.rh, j.frame, j.stats, j.hist, j.matVD, j.nMat, j.W, j.H, j.cam, j.rule, own..., j.outFrame, j.outStats,
                           j.kept);
    };
    switch ((j.bilinear ? 4 : 0) | (j.motion ? 2 : 0) | (demod ? 1 : 0)) {
        case 0: launch(k_reproject<false, false, false>); break;
        case 1: launch(k_reproject<false, true, false, float>, j.floorA); break;
        case 2: launch(k_reproject<true, false, false, ReprojMotion, float>, *j.motion, 0.0f); break;
        case 3: launch(k_reproject<true, true, false, ReprojMotion, float>, *j.motion, j.floorA); break;
        case 4: launch(k_reproject<false, false, true, float, float>, j.snap, j.floorA); break;      // kept[1] = the blended pixels
        case 5: launch(k_reproject<false, true, true, float, float>, j.snap, j.floorA); break;
        case 6: launch(k_reproject<true, false, true, float, float, ReprojMotion>, j.snap, j.floorA, *j.motion); break;
        case 7: launch(k_reproject<true, true, true, float, float, ReprojMotion>, j.snap, j.floorA, *j.motion); break;
    }
    if (j.sn) {                                                                            // include/pt_reproject_through.h: the chain pixels, on top
        if (j.motion || demod || j.radius < 0 || j.radius > 4) return hipErrorInvalidValue;
        const int n = j.W * j.H;
        hipLaunchKernelGGL(k_through_pack, dim3((unsigned)((n + TP_B - 1) / TP_B)), dim3(TP_B), 0, s, j.sh, j.yh, j.frame, n, j.pack);
        hipLaunchKernelGGL(k_reproject_chain, grid, block, 0, s, j.sn, j.yn, (const float4*)j.pack, j.frame, j.stats, j.hist, j.matVD, j.nMat, j.W, j.H, j.cam,
                           j.rule, j.pointTol, j.radius, j.outFrame, j.outStats, j.kept);
    }
    return hipGetLastError();
}

hipError_t validateLaunch(const ValidateJob& j, hipStream_t s) {
    hipError_t e = hipMemsetAsync(j.reduced, 0, 4, s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((j.W + RP_BX - 1) / RP_BX), (unsigned)((j.H + RP_BY - 1) / RP_BY)), block(RP_BX, RP_BY);
    const ValidateRule r{j.zLo, j.zHi, j.normalTol, j.overlay[0], j.overlay[1], j.overlay[2]};
#define VL_ARGS j.feat, j.frame, j.stats, j.heldFrame, j.heldStats, j.W, j.H, r, j.outFrame, j.outStats, j.kappa, j.reduced
    if (j.radius == 1) hipLaunchKernelGGL(k_history_merge<1>, grid, block, 0, s, VL_ARGS);
    else if (j.radius == 2) hipLaunchKernelGGL(k_history_merge<2>, grid, block, 0, s, VL_ARGS);
    else if (j.radius == 3) hipLaunchKernelGGL(k_history_merge<3>, grid, block, 0, s, VL_ARGS);
    else if (j.radius == 4) hipLaunchKernelGGL(k_history_merge<4>, grid, block, 0, s, VL_ARGS);
    else return hipErrorInvalidValue;
#undef VL_ARGS
    return hipGetLastError();
}
