// pt_geom_steps.hpp — the steps that the geometry units share: pt_pose.hip, pt_skin.hip, pt_skin_dq.hip, pt_rig.hip, pt_rig_mix.hip, pt_rig_ik.hip, pt_morph.hip and pt_normals.hip include
// it after <hip/hip_runtime.h>, and nobody else does.  Not a launch header: the host half of the pose never sees it, and no render kernel is
// here, so kernel_source_hash() does not cover it.  Every unit that includes it is compiled with -ffp-contract=off, so each a * b + c below is
// a rounded product and a rounded sum, in the order written: the CPU statements of the *_rule.hpp files are the specification of that order.
#pragma once
#include <cstdint>

namespace {

constexpr int BLOCK = 256;

// the blocks of a launch of one lane per item; false: more than a grid's x dimension holds (the launch is refused with hipErrorInvalidValue)
inline bool gridOf(int64_t n, unsigned* blocks) {
    const long long b = ((long long)n + BLOCK - 1) / BLOCK;
    if (b > 0x7fffffffLL) return false;
    *blocks = (unsigned)b;
    return true;
}

// M lies at floats 0-11 of a record, three rows of (m0, m1, m2, t); the fourth float of v is carried through
__device__ __forceinline__ float4 posePoint(const float4 r0, const float4 r1, const float4 r2, const float4 v) {
    return make_float4(((r0.x * v.x + r0.y * v.y) + r0.z * v.z) + r0.w, ((r1.x * v.x + r1.y * v.y) + r1.z * v.z) + r1.w,
                       ((r2.x * v.x + r2.y * v.y) + r2.z * v.z) + r2.w, v.w);
}
// N lies at floats 12-20 of the record: n3 = (n00, n01, n02, n10), n4 = (n11, n12, n20, n21), n22
__device__ __forceinline__ float4 poseNormal(const float4 n3, const float4 n4, const float n22, const float4 v) {
    return make_float4((n3.x * v.x + n3.y * v.y) + n3.z * v.z, (n3.w * v.x + n4.x * v.y) + n4.y * v.z, (n4.z * v.x + n4.w * v.y) + n22 * v.z, v.w);
}

// a blend's first term and each further one, per float
__device__ __forceinline__ float4 scaled(const float w, const float4 x) { return make_float4(w * x.x, w * x.y, w * x.z, w * x.w); }
__device__ __forceinline__ float4 added(const float4 a, const float w, const float4 x) {
    return make_float4(a.x + w * x.x, a.y + w * x.y, a.z + w * x.z, a.w + w * x.w);
}

}  // namespace
