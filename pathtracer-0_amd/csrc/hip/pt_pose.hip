// pt_pose.hip — the kernels of include/pt_pose.h: the device statement of ptp::poseTriangles (pt_pose_rule.hpp), which is their specification.
// A scene-build file like pt_refit.hip and pt_move.hip: no render kernel is here.
//
//   k_pose_quads   one lane per float4 of the six leading ones of a triangle: the part id of its triangle, the three rows of M (lanes 0-2 of a
//                  triangle) or of N (lanes 3-5) from the part's record, one 16-byte load of the rest pose and one 16-byte store; the fourth
//                  float is carried through
//   k_pose_tris    the alternative: one lane per triangle, six float4 loads and stores, the record's six float4 once per lane
//   k_pose_gather  one lane per wanted row of binding 10: the rows the root and group records need, into one small buffer
//   k_pose_motion  one lane per triangle: the first 48 bytes of the posed triangle into motionPack's record (include/pt_motion.h) — float 3 the moved
//                  flag against the mark's record (0 for the mark's own), floats 7 and 11 zero
// Triangles of part -1 are never written: the destination held the rest pose before the first launch.  Every lane writes its own float4s and
// reads only what the host uploaded or an earlier launch stored: kernel boundaries are the only ordering.  The file is compiled with
// -ffp-contract=off like the rest of the library, so a * b + c is a rounded product and a rounded sum.  Part ids were range-checked on the host
// (checkPoseCreate); row ids are the refit plan's, range-checked by planRefit.
#include <hip/hip_runtime.h>

#include "pt_geom_steps.hpp"
#include "pt_pose_launch.hpp"

namespace {

__global__ void __launch_bounds__(BLOCK) k_pose_quads(const float4* __restrict__ rest, const int32_t* __restrict__ triPart, long long nQuads,
                                                     const float4* __restrict__ xforms, float4* __restrict__ out) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nQuads) return;
    const long long t = i / 6;
    const int q = (int)(i - 6 * t);
    const int p = triPart[t];
    if (p < 0) return;
    const float4* X = xforms + 6 * (size_t)p;
    const size_t at = 10 * (size_t)t + q;
    const float4 v = rest[at];
    out[at] = q < 3 ? posePoint(X[0], X[1], X[2], v) : poseNormal(X[3], X[4], X[5].x, v);
}

__global__ void __launch_bounds__(BLOCK) k_pose_tris(const float4* __restrict__ rest, const int32_t* __restrict__ triPart, long long nTris,
                                                    const float4* __restrict__ xforms, float4* __restrict__ out) {
    const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= nTris) return;
    const int p = triPart[t];
    if (p < 0) return;
    const float4* X = xforms + 6 * (size_t)p;
    const float4 r0 = X[0], r1 = X[1], r2 = X[2], n3 = X[3], n4 = X[4];
    const float n22 = X[5].x;
    const float4* T = rest + 10 * (size_t)t;
    float4* O = out + 10 * (size_t)t;
    const float4 a = T[0], b = T[1], c = T[2], d = T[3], e = T[4], f = T[5];
    O[0] = posePoint(r0, r1, r2, a); O[1] = posePoint(r0, r1, r2, b); O[2] = posePoint(r0, r1, r2, c);
    O[3] = poseNormal(n3, n4, n22, d); O[4] = poseNormal(n3, n4, n22, e); O[5] = poseNormal(n3, n4, n22, f);
}

__global__ void __launch_bounds__(BLOCK) k_pose_gather(const float4* __restrict__ data, const int32_t* __restrict__ ids, int n, float4* __restrict__ out) {
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n) return;
    const size_t row = (size_t)ids[r];
    out[2 * (size_t)r] = data[2 * row];
    out[2 * (size_t)r + 1] = data[2 * row + 1];
}

__global__ void __launch_bounds__(BLOCK) k_pose_motion(const float4* __restrict__ tris, int nTris, const float4* __restrict__ then, int nThen, float4* __restrict__ out) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= nTris) return;
    const float4* T = tris + 10 * (size_t)t;
    const float4 a = T[0], b = T[1], c = T[2];
    int flag = 0;
    if (then) {
        flag = t < nThen ? 0 : 1;
        if (!flag) {
            const float4 p = then[3 * (size_t)t], q = then[3 * (size_t)t + 1], r = then[3 * (size_t)t + 2];
            if (!(a.x == p.x) || !(a.y == p.y) || !(a.z == p.z) || !(b.x == q.x) || !(b.y == q.y) || !(b.z == q.z) || !(c.x == r.x) || !(c.y == r.y) || !(c.z == r.z)) flag = 1;
        }
    }
    float4* o = out + 3 * (size_t)t;
    o[0] = make_float4(a.x, a.y, a.z, __int_as_float(flag));
    o[1] = make_float4(b.x, b.y, b.z, 0.0f);
    o[2] = make_float4(c.x, c.y, c.z, 0.0f);
}

}  // namespace

hipError_t ptPoseMotionLaunch(const float* tris, int nTris, const float4* then, int nThen, float4* out, hipStream_t s) {
    unsigned blocks;
    if (nTris > 0 && gridOf(nTris, &blocks))                     // (an int's worth of lanes always fits a grid)
        hipLaunchKernelGGL(k_pose_motion, dim3(blocks), dim3(BLOCK), 0, s, reinterpret_cast<const float4*>(tris), nTris, then, nThen, out);
    return hipGetLastError();
}

hipError_t ptPoseLaunch(const float* rest, const int32_t* triPart, int64_t nTris, const float* xforms, float* out, PtPoseKernel which, hipStream_t s) {
    if (nTris <= 0) return hipGetLastError();
    const long long n = which == PT_POSE_PER_QUAD ? 6 * (long long)nTris : (long long)nTris;
    unsigned blocks;
    if (!gridOf(n, &blocks)) return hipErrorInvalidValue;
    const float4* r4 = reinterpret_cast<const float4*>(rest); const float4* x4 = reinterpret_cast<const float4*>(xforms); float4* o4 = reinterpret_cast<float4*>(out);
    if (which == PT_POSE_PER_QUAD) hipLaunchKernelGGL(k_pose_quads, dim3(blocks), dim3(BLOCK), 0, s, r4, triPart, n, x4, o4);
    else hipLaunchKernelGGL(k_pose_tris, dim3(blocks), dim3(BLOCK), 0, s, r4, triPart, n, x4, o4);
    return hipGetLastError();
}

hipError_t ptPoseGatherLaunch(const float* data, const int32_t* ids, int n, float* out, hipStream_t s) {
    unsigned blocks;
    if (n > 0 && gridOf(n, &blocks))
        hipLaunchKernelGGL(k_pose_gather, dim3(blocks), dim3(BLOCK), 0, s, reinterpret_cast<const float4*>(data), ids, n, reinterpret_cast<float4*>(out));
    return hipGetLastError();
}
