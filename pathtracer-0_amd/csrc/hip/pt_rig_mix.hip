// pt_rig_mix.hip — the kernel of include/pt_rig_mix.h: the device statement of ptp::rigMix (pt_rig_mix_rule.hpp), which is its specification.
// A scene-build file like pt_rig.hip: no render kernel is here.
//
//   k_rig_mix     one lane per joint.  The layer table lies by value in the kernel arguments and is uniform over the launch, so the loop over the
//                 layers and the tests u == 0, mode and mask != null are wave-uniform branches.  Per layer three 16-byte loads of key ka's local
//                 (three more of kb's when u != 0, three of key 0's for an additive layer, four bytes of the mask when there is one); the tests
//                 on the effective weight e differ from lane to lane and are selects over values every lane computes.  Three 16-byte stores,
//                 the paddings as 0.
// Every lane writes its own float4s and reads only what earlier launches and uploads wrote.  The key and slot indices were checked on the host
// (ptp::checkRigMixLayers).  No LDS, no atomics.  The file is compiled with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt like the
// rest of the library, so a * b + c is a rounded product and a rounded sum, in the order written.
#include <hip/hip_runtime.h>

#include "pt_geom_steps.hpp"
#include "pt_rig_mix_launch.hpp"

namespace {

struct Local { float4 t, q, s; };

__device__ __forceinline__ Local loadLocal(const float* __restrict__ p, size_t j) {
    const float4* __restrict__ v = reinterpret_cast<const float4*>(p);
    return Local{v[3 * j], v[3 * j + 1], v[3 * j + 2]};
}

// step 5 of include/pt_rig.h on one joint: a and b under u, the quaternion along the shorter arc
__device__ __forceinline__ Local blend(const Local& a, const Local& b, float u) {
    const float v = 1.0f - u;
    const float d = ((a.q.x * b.q.x + a.q.y * b.q.y) + a.q.z * b.q.z) + a.q.w * b.q.w;
    const float uq = d < 0.0f ? -u : u;
    return Local{added(scaled(v, a.t), u, b.t), added(scaled(v, a.q), uq, b.q), added(scaled(v, a.s), u, b.s)};
}

// p (x) q on (x y z w), in the header's order
__device__ __forceinline__ float4 quatMul(const float4 p, const float4 q) {
    return make_float4(((p.w * q.x + p.x * q.w) + p.y * q.z) - p.z * q.y, ((p.w * q.y - p.x * q.z) + p.y * q.w) + p.z * q.x,
                       ((p.w * q.z + p.x * q.y) - p.y * q.x) + p.z * q.w, ((p.w * q.w - p.x * q.x) - p.y * q.y) - p.z * q.z);
}

__device__ __forceinline__ float4 pick(bool c, const float4 a, const float4 b) { return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w); }
__device__ __forceinline__ Local pick(bool c, const Local& a, const Local& b) { return Local{pick(c, a.t, b.t), pick(c, a.q, b.q), pick(c, a.s, b.s)}; }

// acc + e * (S - R) per float: the difference, the product, the sum
__device__ __forceinline__ float4 departed(const float4 acc, float e, const float4 S, const float4 R) {
    return make_float4(acc.x + e * (S.x - R.x), acc.y + e * (S.y - R.y), acc.z + e * (S.z - R.z), acc.w + e * (S.w - R.w));
}

__global__ void __launch_bounds__(BLOCK) k_rig_mix(const PtRigMixTable T, int nJoints, float4* __restrict__ out) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nJoints) return;
    const size_t j = (size_t)i;
    Local acc = loadLocal(T.a[0], j);                                   // steps 2 and 4: the base
    if (T.u[0] != 0.0f) acc = blend(acc, loadLocal(T.b[0], j), T.u[0]);
    for (int l = 1; l < T.nLayers; l++) {
        Local S = loadLocal(T.a[l], j);                                 // step 2
        const float u = T.u[l];
        if (u != 0.0f) S = blend(S, loadLocal(T.b[l], j), u);
        const float* __restrict__ mask = T.mask[l];
        float e = T.weight[l];                                          // step 3
        if (mask) e = e * mask[j];
        Local next;
        if (T.mode[l] == 0) {                                           // step 5
            next = pick(e == 1.0f, S, blend(acc, S, e));
        } else {                                                        // step 6
            const Local R = loadLocal(T.r[l], j);
            float4 dq = quatMul(S.q, make_float4(-R.q.x, -R.q.y, -R.q.z, R.q.w));
            if (dq.w < 0.0f) dq = make_float4(-dq.x, -dq.y, -dq.z, -dq.w);
            const float v = 1.0f - e;
            const float4 dp = make_float4(e * dq.x, e * dq.y, e * dq.z, v + e * dq.w);
            next = Local{departed(acc.t, e, S.t, R.t), quatMul(dp, acc.q), departed(acc.s, e, S.s, R.s)};
        }
        acc = pick(e == 0.0f, acc, next);
    }
    out[3 * j] = make_float4(acc.t.x, acc.t.y, acc.t.z, 0.0f);          // step 7
    out[3 * j + 1] = acc.q;
    out[3 * j + 2] = make_float4(acc.s.x, acc.s.y, acc.s.z, 0.0f);
}

}  // namespace

hipError_t ptRigMixLaunch(const PtRigMixTable& table, int nJoints, float* out, hipStream_t s) {
    if (nJoints <= 0) return hipGetLastError();
    if (table.nLayers < 1 || table.nLayers > PT_RIG_MIX_TABLE_LAYERS) return hipErrorInvalidValue;
    unsigned blocks;
    if (!gridOf(nJoints, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rig_mix, dim3(blocks), dim3(BLOCK), 0, s, table, nJoints, reinterpret_cast<float4*>(out));
    return hipGetLastError();
}
