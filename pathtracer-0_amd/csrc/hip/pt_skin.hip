// pt_skin.hip — the kernels of include/pt_skin.h: two device statements of ptp::skinTriangles (pt_skin_rule.hpp), which is their specification.
// A scene-build file like pt_pose.hip: no render kernel is here.
//
//   k_skin_quads    one lane per float4 of the six leading ones of a triangle: lanes 0-2 are the vertices of corners 0-2, lanes 3-5 their normals.
//                   One int4 of bone ids and one float4 of weights for the lane's corner; the three rows of M (vertex lanes) or the nine floats of
//                   N (normal lanes) blended from at most four records; one 16-byte load of the rest pose and one 16-byte store; the fourth float
//                   is carried through
//   k_skin_corners  the alternative: one lane per corner, three per triangle.  The skin words once, all 21 floats blended, the corner's vertex
//                   and its normal posed
// A corner whose slot 0 holds -1 is never written: the destination held the rest pose before the first launch.  The weights of empty slots are
// never multiplied (they may be NaN).  Every lane writes its own float4s and reads only what the host uploaded: kernel boundaries are the only
// ordering.  The records stay in global memory (65536 of them are 6 MB: the L2 serves them).  The file is compiled with -ffp-contract=off like
// the rest of the library, so a + w * x is a rounded product and a rounded sum.  Bone ids were range-checked on the host (checkSkinCreate).
#include <hip/hip_runtime.h>

#include "pt_geom_steps.hpp"
#include "pt_skin_launch.hpp"

namespace {

// the blend of three consecutive float4 of the records (from float4 `first`), slots in order; slot 0 is used
__device__ __forceinline__ void blend3(const float4* __restrict__ xforms, const int first, const int4 b, const float4 w, float4& a0, float4& a1, float4& a2) {
    const float4* X = xforms + 6 * (size_t)b.x + first;
    a0 = scaled(w.x, X[0]); a1 = scaled(w.x, X[1]); a2 = scaled(w.x, X[2]);
    if (b.y < 0) return;
    X = xforms + 6 * (size_t)b.y + first;
    a0 = added(a0, w.y, X[0]); a1 = added(a1, w.y, X[1]); a2 = added(a2, w.y, X[2]);
    if (b.z < 0) return;
    X = xforms + 6 * (size_t)b.z + first;
    a0 = added(a0, w.z, X[0]); a1 = added(a1, w.z, X[1]); a2 = added(a2, w.z, X[2]);
    if (b.w < 0) return;
    X = xforms + 6 * (size_t)b.w + first;
    a0 = added(a0, w.w, X[0]); a1 = added(a1, w.w, X[1]); a2 = added(a2, w.w, X[2]);
}

__global__ void __launch_bounds__(BLOCK) k_skin_quads(const float4* __restrict__ rest, const int4* __restrict__ bone, const float4* __restrict__ weight, long long nQuads,
                                                     const float4* __restrict__ xforms, float4* __restrict__ out) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nQuads) return;
    const long long t = i / 6;
    const int q = (int)(i - 6 * t);
    const int c = q < 3 ? q : q - 3;
    const int4 b = bone[3 * (size_t)t + c];
    if (b.x < 0) return;
    const float4 w = weight[3 * (size_t)t + c];
    float4 a0, a1, a2;
    blend3(xforms, q < 3 ? 0 : 3, b, w, a0, a1, a2);               // (a normal lane blends floats 21-23 too: the padding, never used)
    const size_t at = 10 * (size_t)t + q;
    const float4 v = rest[at];
    out[at] = q < 3 ? posePoint(a0, a1, a2, v) : poseNormal(a0, a1, a2.x, v);      // (pt_pose.hip's arithmetic, on the blended rows)
}

__global__ void __launch_bounds__(BLOCK) k_skin_corners(const float4* __restrict__ rest, const int4* __restrict__ bone, const float4* __restrict__ weight, long long nCorners,
                                                       const float4* __restrict__ xforms, float4* __restrict__ out) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nCorners) return;
    const int4 b = bone[i];
    if (b.x < 0) return;
    const float4 w = weight[i];
    const long long t = i / 3;
    const int c = (int)(i - 3 * t);
    float4 r0, r1, r2, n3, n4, n5;
    blend3(xforms, 0, b, w, r0, r1, r2);
    blend3(xforms, 3, b, w, n3, n4, n5);
    const size_t at = 10 * (size_t)t + c;
    const float4 v = rest[at], n = rest[at + 3];
    out[at] = posePoint(r0, r1, r2, v);
    out[at + 3] = poseNormal(n3, n4, n5.x, n);
}

}  // namespace

hipError_t ptSkinLaunch(const float* rest, const int32_t* bone, const float* weight, int64_t nTris, const float* xforms, float* out, PtSkinKernel which, hipStream_t s) {
    if (nTris <= 0) return hipGetLastError();
    const long long n = (which == PT_SKIN_PER_QUAD ? 6 : 3) * (long long)nTris;
    unsigned blocks;
    if (!gridOf(n, &blocks)) return hipErrorInvalidValue;
    const float4* r4 = reinterpret_cast<const float4*>(rest); const float4* x4 = reinterpret_cast<const float4*>(xforms); float4* o4 = reinterpret_cast<float4*>(out);
    const int4* b4 = reinterpret_cast<const int4*>(bone); const float4* w4 = reinterpret_cast<const float4*>(weight);
    if (which == PT_SKIN_PER_QUAD) hipLaunchKernelGGL(k_skin_quads, dim3(blocks), dim3(BLOCK), 0, s, r4, b4, w4, n, x4, o4);
    else hipLaunchKernelGGL(k_skin_corners, dim3(blocks), dim3(BLOCK), 0, s, r4, b4, w4, n, x4, o4);
    return hipGetLastError();
}
