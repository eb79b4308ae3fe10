// pt_rig.hip — the kernels of include/pt_rig.h: the device statements of ptp::rigBlend and of ptp::rigLocal / rigCompose / rigRecord
// (pt_rig_rule.hpp), which are their specification.  A scene-build file like pt_skin_dq.hip: no render kernel is here.
//
//   k_rig_blend   one lane per joint: three 16-byte loads from each of two keys, the shorter-arc lerp, three 16-byte stores
//   k_rig_level   one lane per joint of one level.  Its id from the level's slice of the (depth, id) order; three 16-byte loads of its local, the
//                 local matrix in registers; a root keeps it, any other joint loads its parent's world matrix (three 16-byte loads, written by the
//                 launch before) and composes; three 16-byte stores of W; with bind matrices three more loads and a second composition; the
//                 cofactors, the determinant, and six 16-byte stores of the record
// Every lane writes its own float4s.  A level reads what the level before it wrote on the same stream: kernel boundaries are the only ordering.
// The ids were range-checked on the host (checkRigCreate), the order and the level starts are the host plan's (ptp::rigPlan).  The file is
// compiled with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt like the rest of the library, so a * b + c is a rounded product and
// a rounded sum, and sqrtf and / are the correctly rounded ones.
#include <hip/hip_runtime.h>

#include "pt_geom_steps.hpp"
#include "pt_rig_launch.hpp"

namespace {

// a 3 x 4 matrix as its rows (m_i0, m_i1, m_i2, m_i3)
struct Mat34 { float4 r0, r1, r2; };

// one row of A o B: the linear part, and the translation with a's own added last
__device__ __forceinline__ float4 composeRow(const float4 a, const Mat34& B) {
    return make_float4((a.x * B.r0.x + a.y * B.r1.x) + a.z * B.r2.x, (a.x * B.r0.y + a.y * B.r1.y) + a.z * B.r2.y, (a.x * B.r0.z + a.y * B.r1.z) + a.z * B.r2.z,
                       ((a.x * B.r0.w + a.y * B.r1.w) + a.z * B.r2.w) + a.w);
}
__device__ __forceinline__ Mat34 compose(const Mat34& A, const Mat34& B) { return Mat34{composeRow(A.r0, B), composeRow(A.r1, B), composeRow(A.r2, B)}; }

__device__ __forceinline__ Mat34 loadMat(const float4* __restrict__ p, size_t j) { return Mat34{p[3 * j], p[3 * j + 1], p[3 * j + 2]}; }

__global__ void __launch_bounds__(BLOCK) k_rig_blend(const float4* __restrict__ a, const float4* __restrict__ b, float u, int nJoints, float4* __restrict__ out) {
    const long long j = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= nJoints) return;
    const float v = 1.0f - u;
    const float4 ta = a[3 * (size_t)j], qa = a[3 * (size_t)j + 1], sa = a[3 * (size_t)j + 2];
    const float4 tb = b[3 * (size_t)j], qb = b[3 * (size_t)j + 1], sb = b[3 * (size_t)j + 2];
    const float d = ((qa.x * qb.x + qa.y * qb.y) + qa.z * qb.z) + qa.w * qb.w;
    const float uq = d < 0.0f ? -u : u;
    out[3 * (size_t)j] = added(scaled(v, ta), u, tb);
    out[3 * (size_t)j + 1] = added(scaled(v, qa), uq, qb);
    out[3 * (size_t)j + 2] = added(scaled(v, sa), u, sb);
}

__global__ void __launch_bounds__(BLOCK) k_rig_level(const int32_t* __restrict__ order, int first, int count, const int32_t* __restrict__ parent,
                                                    const float4* __restrict__ locals, const float4* __restrict__ invBind, float4* world, float4* __restrict__ records) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= count) return;
    const size_t j = (size_t)order[(size_t)first + (size_t)i];
    // step 1
    const float4 t = locals[3 * j], q = locals[3 * j + 1], s = locals[3 * j + 2];
    const float n = sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w);
    const float x = q.x / n, y = q.y / n, z = q.z / n, w = q.w / n;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    Mat34 W;
    W.r0 = make_float4((1.0f - 2.0f * (yy + zz)) * s.x, (2.0f * (xy - wz)) * s.y, (2.0f * (xz + wy)) * s.z, t.x);
    W.r1 = make_float4((2.0f * (xy + wz)) * s.x, (1.0f - 2.0f * (xx + zz)) * s.y, (2.0f * (yz - wx)) * s.z, t.y);
    W.r2 = make_float4((2.0f * (xz - wy)) * s.x, (2.0f * (yz + wx)) * s.y, (1.0f - 2.0f * (xx + yy)) * s.z, t.z);
    // step 2: a root keeps its local matrix
    const int p = parent[j];
    if (p >= 0) W = compose(loadMat(world, (size_t)p), W);
    world[3 * j] = W.r0; world[3 * j + 1] = W.r1; world[3 * j + 2] = W.r2;
    // step 3
    Mat34 M = W;
    if (invBind) M = compose(W, loadMat(invBind, j));
    // step 4
    const float c00 = M.r1.y * M.r2.z - M.r1.z * M.r2.y, c01 = M.r1.z * M.r2.x - M.r1.x * M.r2.z, c02 = M.r1.x * M.r2.y - M.r1.y * M.r2.x;
    const float c10 = M.r2.y * M.r0.z - M.r2.z * M.r0.y, c11 = M.r2.z * M.r0.x - M.r2.x * M.r0.z, c12 = M.r2.x * M.r0.y - M.r2.y * M.r0.x;
    const float c20 = M.r0.y * M.r1.z - M.r0.z * M.r1.y, c21 = M.r0.z * M.r1.x - M.r0.x * M.r1.z, c22 = M.r0.x * M.r1.y - M.r0.y * M.r1.x;
    const float det = (M.r0.x * c00 + M.r0.y * c01) + M.r0.z * c02;
    records[6 * j] = M.r0; records[6 * j + 1] = M.r1; records[6 * j + 2] = M.r2;
    records[6 * j + 3] = make_float4(c00 / det, c01 / det, c02 / det, c10 / det);
    records[6 * j + 4] = make_float4(c11 / det, c12 / det, c20 / det, c21 / det);
    records[6 * j + 5] = make_float4(c22 / det, 0.0f, 0.0f, 0.0f);
}

}  // namespace

hipError_t ptRigBlendLaunch(const float* a, const float* b, float u, int nJoints, float* out, hipStream_t s) {
    if (nJoints <= 0) return hipGetLastError();
    unsigned blocks;
    if (!gridOf(nJoints, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rig_blend, dim3(blocks), dim3(BLOCK), 0, s, reinterpret_cast<const float4*>(a), reinterpret_cast<const float4*>(b), u, nJoints,
                       reinterpret_cast<float4*>(out));
    return hipGetLastError();
}

hipError_t ptRigLevelLaunch(const int32_t* order, int first, int count, const int32_t* parent, const float* locals, const float* invBind, float* world, float* records,
                            hipStream_t s) {
    if (count <= 0) return hipGetLastError();
    unsigned blocks;
    if (!gridOf(count, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rig_level, dim3(blocks), dim3(BLOCK), 0, s, order, first, count, parent, reinterpret_cast<const float4*>(locals),
                       reinterpret_cast<const float4*>(invBind), reinterpret_cast<float4*>(world), reinterpret_cast<float4*>(records));
    return hipGetLastError();
}
