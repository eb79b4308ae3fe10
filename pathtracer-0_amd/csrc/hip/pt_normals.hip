// pt_normals.hip — the kernels of include/pt_normals.h: the device statement of ptp::smoothNormals (pt_normals_rule.hpp), which is their
// specification.  A scene-build file like pt_pose.hip, pt_skin.hip and pt_morph.hip: no render kernel is here.
//
//   k_normals_faces           one lane per LISTED triangle (one with at least one id >= 0).  Three 16-byte vertex loads from the posed triangles, one
//                             16-byte store into the face-vector array, indexed by triangle id (the fourth float is 0).
//   k_normals_gather_vertex   one lane per NON-EMPTY vertex.  It walks its row of corners (ascending), sums their triangles' face vectors in
//                             that order, normalises once and stores 12 bytes to each of its corners (a second walk of the row).
//   k_normals_gather_corner   one lane per corner with an id >= 0.  It walks its vertex's row itself, sums and normalises as above and stores
//                             its own 12 bytes: the sums are made once per corner instead of once per vertex, but every store is the lane's own.
// Both gathers call the same normalsOfRow, so they give the same bits by construction.  An inverted-index sum: per destination a list in a fixed
// order, so the bits do not depend on the launch.  A wave runs as long as its longest row, and a fan centre has a long one; rows are not split,
// because the order of the sum is the rule (scripts/normals_probe.py measures a table with one long row).  The row is walked four entries a step
// with no branch inside the step, as k_morph_corners walks its own: the corner ids, then the face vectors of all four are in flight before the
// first sum.  A row whose length is not finite and > 0 stores nothing: its corners keep what the pose's rule wrote.  Vector loads and stores only,
// no atomics: kernel boundaries are the only ordering (the faces launch ends before the gather starts; the gather reads faces and the index and
// writes normals, which no lane of it reads).  The file is compiled with -ffp-contract=off and the correctly rounded divide and square root like
// the rest of the library.  Every index was range-checked on the host (checkNormalsAttach, normalRows).
#include <hip/hip_runtime.h>

#include "pt_geom_steps.hpp"
#include "pt_normals_launch.hpp"

namespace {

__global__ void __launch_bounds__(BLOCK) k_normals_faces(const float4* __restrict__ dst, const int* __restrict__ tris, long long nListed, int flip,
                                                        float4* __restrict__ faces) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nListed) return;
    const int t = tris[i];
    const float4* v = dst + 10 * (size_t)t;
    const float4 v0 = v[0], v1 = v[1], v2 = v[2];
    const float e1x = v1.x - v0.x, e1y = v1.y - v0.y, e1z = v1.z - v0.z;
    const float e2x = v2.x - v0.x, e2y = v2.y - v0.y, e2z = v2.z - v0.z;
    float4 F;
    F.x = e1y * e2z - e1z * e2y;
    F.y = e1z * e2x - e1x * e2z;
    F.z = e1x * e2y - e1y * e2x;
    F.w = 0.0f;
    if (flip) { F.x = -F.x; F.y = -F.y; F.z = -F.z; }
    faces[t] = F;
}

__device__ __forceinline__ void faceAdd(float4& S, const bool there, const float4 F) {
    S.x = there ? S.x + F.x : S.x; S.y = there ? S.y + F.y : S.y; S.z = there ? S.z + F.z : S.z;
}

// THE RULE, steps 2-4, over the row [first, end) of corners (end > first): false where the fallback applies
__device__ __forceinline__ bool normalsOfRow(const float4* __restrict__ faces, const int* __restrict__ corners, const int first, const int end, float4& N) {
    float4 S = faces[corners[first] / 3];
    // four entries a step, in the row's order; where the row has ended its last entry is loaded again (every index stays inside the row) and is
    // not added again
    for (int j = first + 1; j < end; j += 4) {
        const int m = end - j;
        const int* c = corners + j;
        const int i1 = m > 1 ? 1 : 0, i2 = m > 2 ? 2 : i1, i3 = m > 3 ? 3 : i2;
        const int q0 = c[0], q1 = c[i1], q2 = c[i2], q3 = c[i3];
        const float4 F0 = faces[q0 / 3], F1 = faces[q1 / 3], F2 = faces[q2 / 3], F3 = faces[q3 / 3];
        faceAdd(S, true, F0);
        faceAdd(S, m > 1, F1);
        faceAdd(S, m > 2, F2);
        faceAdd(S, m > 3, F3);
    }
    const float xx = S.x * S.x, yy = S.y * S.y, zz = S.z * S.z;
    const float L = sqrtf((xx + yy) + zz);
    // (finite and > 0, without isfinite: a NaN compares false, an infinity is not below the largest float's successor)
    if (!(L > 0.0f && L <= 3.402823466e+38f)) return false;
    N.x = S.x / L; N.y = S.y / L; N.z = S.z / L;
    return true;
}

// floats 12+4c .. 12+4c+2 of corner q: 12 bytes, the fourth float stays
__device__ __forceinline__ void storeNormal(float* __restrict__ dst, const int q, const float4 N) {
    const int t = q / 3;
    float* p = dst + 40 * (size_t)t + 12 + 4 * (q - 3 * t);
    p[0] = N.x; p[1] = N.y; p[2] = N.z;
}

__global__ void __launch_bounds__(BLOCK) k_normals_gather_vertex(const float4* __restrict__ faces, const int* __restrict__ rowStart, long long nRows,
                                                                const int* __restrict__ corners, float* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nRows) return;
    const int first = rowStart[i], end = rowStart[i + 1];
    float4 N;
    if (!normalsOfRow(faces, corners, first, end, N)) return;
    for (int j = first; j < end; j++) storeNormal(dst, corners[j], N);
}

__global__ void __launch_bounds__(BLOCK) k_normals_gather_corner(const float4* __restrict__ faces, const int* __restrict__ rowStart, const int* __restrict__ corners,
                                                                const int* __restrict__ cornerRow, long long nEntries, float* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nEntries) return;
    const int r = cornerRow[i];
    float4 N;
    if (!normalsOfRow(faces, corners, rowStart[r], rowStart[r + 1], N)) return;
    storeNormal(dst, corners[i], N);
}

}  // namespace

hipError_t ptNormalsFacesLaunch(const float* dst, const int32_t* tris, int64_t nListed, int flip, float* faces, hipStream_t s) {
    if (nListed <= 0) return hipGetLastError();
    unsigned blocks;
    if (!gridOf(nListed, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_normals_faces, dim3(blocks), dim3(BLOCK), 0, s, reinterpret_cast<const float4*>(dst), tris, (long long)nListed, flip,
                       reinterpret_cast<float4*>(faces));
    return hipGetLastError();
}

hipError_t ptNormalsGatherLaunch(const float* faces, const int32_t* rowStart, int64_t nRows, const int32_t* corners, const int32_t* cornerRow, int64_t nEntries,
                                 float* dst, PtNormalsKernel which, hipStream_t s) {
    if (nRows <= 0 || nEntries <= 0) return hipGetLastError();
    unsigned blocks;
    if (which == PT_NORMALS_PER_VERTEX) {
        if (!gridOf(nRows, &blocks)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_normals_gather_vertex, dim3(blocks), dim3(BLOCK), 0, s, reinterpret_cast<const float4*>(faces), rowStart, (long long)nRows, corners, dst);
    } else {
        if (!gridOf(nEntries, &blocks)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_normals_gather_corner, dim3(blocks), dim3(BLOCK), 0, s, reinterpret_cast<const float4*>(faces), rowStart, corners, cornerRow,
                           (long long)nEntries, dst);
    }
    return hipGetLastError();
}
