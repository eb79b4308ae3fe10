// pt_move.hip — the kernels of the in-place move of a scene's triangles (include/pt_move.h): the device statement of ptl::applyMove
// (pt_scene_move.hpp), which is their specification.  A scene-build file like pt_refit.hip: no render kernel is here.
//
//   k_move_check   one lane per triangle record: the material index of the triangle it references, held to [0, nMat) (layoutScene's refusal)
//   k_move_tris    one lane per triangle record: the id from the record's float 9, the first 48 bytes of the 160-byte triangle as three float4,
//                  v1, e1, e2 stored as two float4 and one float; float 9 (id, last-in-leaf bit) and the padding are not written
//   k_move_shade   one lane per triangle id: floats 12-36 of the triangle into the four float4 of its shading record
//   k_move_nodes   one lane per inner record: its two children's rows of binding 10 (a float4 and a float2 each) into the box floats of the 64-byte
//                  record and of the 80- or 64-byte record of the hand-written kernel; references and padding are not written
// Every lane writes its own record and reads only what earlier launches (the refit's, on a stream the host has synchronised) stored: kernel
// boundaries are the only ordering, there is no hand-off between blocks.  The flags are plain stores of 1 by whoever finds a reason.  The
// subtractions are the host's binary32 subtractions (the file is compiled with -ffp-contract=off like the rest of the library; there is nothing to
// contract anyway), so inf - inf gives the NaN the host gives.  Every index a kernel follows was range-checked on the host: triangle ids by
// layoutScene when the records were built, node ids by planRefit for the tree the topology digest says is the context's.
#include <hip/hip_runtime.h>

#include "pt_move_launch.hpp"

#include <climits>

namespace {

constexpr int BLOCK = 256;

// ptl::toInt: what the x86 conversion returns, INT_MIN for a NaN and for values outside int's range
__device__ __forceinline__ int toInt(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT_MIN; }

__device__ __forceinline__ unsigned recordTriangle(const float4* __restrict__ triRecs, int i) {
    return __float_as_uint(triRecs[3 * (size_t)i + 2].y) & 0x7fffffffu;
}

__global__ void __launch_bounds__(BLOCK) k_move_check(const float4* __restrict__ triRecs, int nTriRecs, const float* __restrict__ tris, int nMat, int* flag) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nTriRecs) return;
    const int mat = toInt(tris[40 * (size_t)recordTriangle(triRecs, i) + 36]);
    if (mat < 0 || mat >= nMat) *flag = 1;
}

__global__ void __launch_bounds__(BLOCK) k_move_tris(float4* triRecs, int nTriRecs, const float* __restrict__ tris) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nTriRecs) return;
    float4* rec = triRecs + 3 * (size_t)i;
    const unsigned t = __float_as_uint(rec[2].y) & 0x7fffffffu;
    const float4* T = reinterpret_cast<const float4*>(tris + 40 * (size_t)t);
    const float4 a = T[0], b = T[1], c = T[2];          // v1 (floats 0-2), v2 (4-6), v3 (8-10)
    const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z, e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
    rec[0] = make_float4(a.x, a.y, a.z, e1x);
    rec[1] = make_float4(e1y, e1z, e2x, e2y);
    reinterpret_cast<float*>(rec + 2)[0] = e2z;
}

__global__ void __launch_bounds__(BLOCK) k_move_shade(float4* shade, int nTris, const float* __restrict__ tris) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= nTris) return;
    const float4* T = reinterpret_cast<const float4*>(tris + 40 * (size_t)t);
    const float4 q3 = T[3], q4 = T[4], q6 = T[6], q7 = T[7], q8 = T[8], q9 = T[9];      // floats 12-15, 16-19, 24-27, 28-31, 32-35, 36-39
    float4* r = shade + 4 * (size_t)t;
    r[0] = make_float4(q3.x, q3.y, q3.z, q4.x);                            // T[12], T[13], T[14], T[16]
    r[1] = make_float4(q4.y, q4.z, q6.x, q6.y);                            // T[17], T[18], T[24], T[25]
    r[2] = make_float4(q7.x, q7.y, q8.x, __int_as_float(toInt(q9.x)));     // T[28], T[29], T[32], the material index
    r[3] = make_float4(q8.y, 0.0f, 0.0f, 0.0f);                            // T[33]
}

template <int STRIDE>
__global__ void __launch_bounds__(BLOCK) k_move_nodes(float4* nodes, float* nodes80, int nInner, const int32_t* __restrict__ child, const float* __restrict__ data, int* flag) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= nInner) return;
    const int2 ch = reinterpret_cast<const int2*>(child)[k];
    const float* ra = data + 8 * (size_t)ch.x; const float* rb = data + 8 * (size_t)ch.y;
    const float4 a0 = *reinterpret_cast<const float4*>(ra); const float2 a1 = *reinterpret_cast<const float2*>(ra + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(rb); const float2 b1 = *reinterpret_cast<const float2*>(rb + 4);
    const float A[6] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y}, B[6] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y};
    float4* n = nodes + 4 * (size_t)k;
    n[0] = make_float4(A[0], B[0], A[1], B[1]); n[1] = make_float4(A[2], B[2], A[3], B[3]); n[2] = make_float4(A[4], B[4], A[5], B[5]);
    float* o = nodes80 + (size_t)(STRIDE / 4) * k;
    if (STRIDE == 80) {                                  // floats 2-19: per axis (Lmin, Rmin | Lmax, Rmax | Lmin, Rmin)
        *reinterpret_cast<float2*>(o + 2) = make_float2(A[0], B[0]);
        *reinterpret_cast<float4*>(o + 4) = make_float4(A[3], B[3], A[0], B[0]);
        *reinterpret_cast<float4*>(o + 8) = make_float4(A[1], B[1], A[4], B[4]);
        *reinterpret_cast<float4*>(o + 12) = make_float4(A[1], B[1], A[2], B[2]);
        *reinterpret_cast<float4*>(o + 16) = make_float4(A[5], B[5], A[2], B[2]);
    } else {                                             // floats 4-15: per axis (Lmin, Rmin | Lmax, Rmax)
        *reinterpret_cast<float4*>(o + 4) = make_float4(A[0], B[0], A[3], B[3]);
        *reinterpret_cast<float4*>(o + 8) = make_float4(A[1], B[1], A[4], B[4]);
        *reinterpret_cast<float4*>(o + 12) = make_float4(A[2], B[2], A[5], B[5]);
    }
    bool ordered = true;
    for (int ax = 0; ax < 3; ax++) if (!(A[ax] <= A[3 + ax]) || !(B[ax] <= B[3 + ax])) ordered = false;
    if (!ordered) *flag = 1;
}

inline unsigned blocksFor(int n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

}  // namespace

hipError_t ptMoveCheckLaunch(const float4* triRecs, int nTriRecs, const float* tris, int nMat, int* flag, hipStream_t s) {
    hipError_t e = hipMemsetAsync(flag, 0, 4, s);
    if (e != hipSuccess) return e;
    if (nTriRecs > 0) hipLaunchKernelGGL(k_move_check, dim3(blocksFor(nTriRecs)), dim3(BLOCK), 0, s, triRecs, nTriRecs, tris, nMat, flag);
    return hipGetLastError();
}

hipError_t ptMovePatchLaunch(const PtMovePatch& p, hipStream_t s) {
    hipError_t e = hipMemsetAsync(p.flag, 0, 4, s);
    if (e != hipSuccess) return e;
    if (p.stride != 80 && p.stride != 64) return hipErrorInvalidValue;
    if (p.nTriRecs > 0) hipLaunchKernelGGL(k_move_tris, dim3(blocksFor(p.nTriRecs)), dim3(BLOCK), 0, s, p.triRecs, p.nTriRecs, p.tris);
    if (p.nTris > 0) hipLaunchKernelGGL(k_move_shade, dim3(blocksFor(p.nTris)), dim3(BLOCK), 0, s, p.shade, p.nTris, p.tris);
    if (p.nInner > 0) {
        if (p.stride == 80) hipLaunchKernelGGL(k_move_nodes<80>, dim3(blocksFor(p.nInner)), dim3(BLOCK), 0, s, p.nodes, p.nodes80, p.nInner, p.child, p.data, p.flag);
        else hipLaunchKernelGGL(k_move_nodes<64>, dim3(blocksFor(p.nInner)), dim3(BLOCK), 0, s, p.nodes, p.nodes80, p.nInner, p.child, p.data, p.flag);
    }
    return hipGetLastError();
}
