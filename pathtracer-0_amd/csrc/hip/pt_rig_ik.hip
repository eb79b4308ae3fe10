// pt_rig_ik.hip — the kernel of include/pt_rig_ik.h: the device statement of ptp::rigIk (pt_rig_ik_rule.hpp).  The steps of one constraint are
// pt_rig_ik_steps.hpp's, the same text the CPU statement compiles.  A scene-build file like pt_rig_mix.hip: no render kernel is here.
//
//   k_rig_ik      one lane per constraint.  One 16-byte load of its row (the joints, found on the host at the attach: no lane walks the
//                 hierarchy), two of its constraint, two of its goal; three of the world matrix of the first joint's parent unless that joint is
//                 a root; then a TWO_BONE lane loads the three locals of root and of mid and the tip's translation and stores one float4 each
//                 into root and mid, an AIM lane loads its joint's three and stores one.  The kind differs from lane to lane: a wave that
//                 holds both runs both branches (the table is not sorted by kind: a launch is one lane per constraint, and a character has a
//                 handful).  A lane whose constraint is left as it is stores nothing.
// The constraints are independent (ptp::checkRigIkAttach), so no lane reads a joint another lane writes, and `in` and `out` may be one array:
// neither is __restrict__.  The joint ids were range-checked on the host.  No LDS, no atomics.  Compiled with -ffp-contract=off
// -fhip-fp32-correctly-rounded-divide-sqrt like the rest of the library.
#include <hip/hip_runtime.h>

#include "pt_geom_steps.hpp"
#include "pt_rig_ik_launch.hpp"
#include "pt_rig_ik_steps.hpp"

namespace {

__device__ __forceinline__ void spread(const float4 a, const float4 b, const float4 c, float* o) {
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w; o[8] = c.x; o[9] = c.y; o[10] = c.z; o[11] = c.w;
}

__global__ void __launch_bounds__(BLOCK) k_rig_ik(const int4* __restrict__ rows, const float4* __restrict__ cons, const float4* __restrict__ goals, int nConstraints,
                                                 const float4* __restrict__ world, const float4* in, float4* out) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nConstraints) return;
    const size_t k = (size_t)i;
    const int4 row = rows[k];
    const float4 head = cons[2 * k], axis4 = cons[2 * k + 1], g0 = goals[2 * k], g1 = goals[2 * k + 1];
    const int kind = __float_as_int(head.x), flags = __float_as_int(head.z);
    const float target[3] = {g0.x, g0.y, g0.z}, pole[3] = {g1.x, g1.y, g1.z};
    const float weight = g0.w;
    float P[12];
    const bool hasP = row.x >= 0;
    if (hasP) spread(world[3 * (size_t)row.x], world[3 * (size_t)row.x + 1], world[3 * (size_t)row.x + 2], P);
    const size_t a = (size_t)row.y;
    float first[12];
    spread(in[3 * a], in[3 * a + 1], in[3 * a + 2], first);
    if (kind == 1) {                                                    // PT_RIG_IK_AIM
        const float axis[3] = {axis4.x, axis4.y, axis4.z};
        float q[4];
        if (ptik::aim(P, hasP, first, axis, target, weight, q)) out[3 * a + 1] = make_float4(q[0], q[1], q[2], q[3]);
        return;
    }
    const size_t b = (size_t)row.z, c = (size_t)row.w;
    float mid[12];
    spread(in[3 * b], in[3 * b + 1], in[3 * b + 2], mid);
    const float4 tt = in[3 * c];
    const float tipT[3] = {tt.x, tt.y, tt.z};
    float q0[4], q1[4];
    if (ptik::twoBone(P, hasP, first, mid, tipT, target, pole, (flags & 1) != 0, weight, q0, q1)) {
        out[3 * a + 1] = make_float4(q0[0], q0[1], q0[2], q0[3]);
        out[3 * b + 1] = make_float4(q1[0], q1[1], q1[2], q1[3]);
    }
}

}  // namespace

hipError_t ptRigIkLaunch(const int32_t* rows, const void* constraints, const void* goals, int nConstraints, const float* world, const float* in, float* out, hipStream_t s) {
    if (nConstraints <= 0) return hipGetLastError();
    unsigned blocks;
    if (!gridOf(nConstraints, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rig_ik, dim3(blocks), dim3(BLOCK), 0, s, reinterpret_cast<const int4*>(rows), reinterpret_cast<const float4*>(constraints),
                       reinterpret_cast<const float4*>(goals), nConstraints, reinterpret_cast<const float4*>(world), reinterpret_cast<const float4*>(in),
                       reinterpret_cast<float4*>(out));
    return hipGetLastError();
}
