// pt_skin_dq.hip — the kernels of include/pt_skin_dq.h: the device statements of ptp::dqFromRecord and of ptp::skinDqTriangles
// (pt_skin_dq_rule.hpp), which are their specification.  A scene-build file like pt_skin.hip: no render kernel is here.
//
//   k_dq_records       one lane per record: three 16-byte loads (the rows of M; N and the padding are not read), the conversion, two 16-byte
//                      stores into the pose's table of dual quaternions (32 bytes per record)
//   k_skin_dq_corners  one lane per corner, three per triangle.  One int4 of bone ids and one float4 of weights; two float4 of the table per used
//                      slot; the blend, the normalisation and the record B held in registers; two 16-byte loads of the rest pose and two stores
// A corner whose slot 0 holds -1 is never written: the destination held the rest pose before the first launch.  The weights of empty slots are
// never multiplied (they may be NaN).  Every lane writes its own float4s; the table is written by the first launch and read by the second on the
// same stream: kernel boundaries are the only ordering.  The table stays in global memory (65536 records are 2 MB: the L2 serves them).  The file
// is compiled with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt like the rest of the library, so a + w * x is a rounded product and
// a rounded sum, and sqrtf and / are the correctly rounded ones.  Bone ids were range-checked on the host (checkSkinCreate).
#include <hip/hip_runtime.h>

#include "pt_geom_steps.hpp"
#include "pt_skin_dq_launch.hpp"

namespace {

__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }

// one more slot onto the blend: the weight negated where the slot's real part lies across from the pivot's
__device__ __forceinline__ void blendSlot(const float4* __restrict__ table, const int b, float w, const float4 pivot, float4& br, float4& bd) {
    const float4 qr = table[2 * (size_t)b], qd = table[2 * (size_t)b + 1];
    if (dot4(pivot, qr) < 0.0f) w = -w;
    br = added(br, w, qr);
    bd = added(bd, w, qd);
}

__global__ void __launch_bounds__(BLOCK) k_dq_records(const float4* __restrict__ xforms, int nParts, float4* __restrict__ table) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nParts) return;
    const float4 r0 = xforms[6 * (size_t)i], r1 = xforms[6 * (size_t)i + 1], r2 = xforms[6 * (size_t)i + 2];
    const float m00 = r0.x, m01 = r0.y, m02 = r0.z, tx = r0.w, m10 = r1.x, m11 = r1.y, m12 = r1.z, ty = r1.w, m20 = r2.x, m21 = r2.y, m22 = r2.z, tz = r2.w;
    const float tr = (m00 + m11) + m22;
    float w, x, y, z;
    if (tr > 0.0f) {
        const float s = sqrtf(tr + 1.0f) * 2.0f;
        w = 0.25f * s; x = (m21 - m12) / s; y = (m02 - m20) / s; z = (m10 - m01) / s;
    } else if (m00 > m11 && m00 > m22) {
        const float s = sqrtf(((1.0f + m00) - m11) - m22) * 2.0f;
        w = (m21 - m12) / s; x = 0.25f * s; y = (m01 + m10) / s; z = (m02 + m20) / s;
    } else if (m11 > m22) {
        const float s = sqrtf(((1.0f + m11) - m00) - m22) * 2.0f;
        w = (m02 - m20) / s; x = (m01 + m10) / s; y = 0.25f * s; z = (m12 + m21) / s;
    } else {
        const float s = sqrtf(((1.0f + m22) - m00) - m11) * 2.0f;
        w = (m10 - m01) / s; x = (m02 + m20) / s; y = (m12 + m21) / s; z = 0.25f * s;
    }
    const float n = sqrtf(((w * w + x * x) + y * y) + z * z);
    w = w / n; x = x / n; y = y / n; z = z / n;
    table[2 * (size_t)i] = make_float4(w, x, y, z);
    table[2 * (size_t)i + 1] = make_float4(-0.5f * ((tx * x + ty * y) + tz * z), 0.5f * ((tx * w + ty * z) - tz * y), 0.5f * ((ty * w + tz * x) - tx * z),
                                           0.5f * ((tz * w + tx * y) - ty * x));
}

__global__ void __launch_bounds__(BLOCK) k_skin_dq_corners(const float4* __restrict__ rest, const int4* __restrict__ bone, const float4* __restrict__ weight, long long nCorners,
                                                          const float4* __restrict__ table, float4* __restrict__ out) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nCorners) return;
    const int4 b = bone[i];
    if (b.x < 0) return;
    const float4 wt = weight[i];
    const long long tri = i / 3;
    const int c = (int)(i - 3 * tri);
    const float4 pivot = table[2 * (size_t)b.x];
    float4 br = scaled(wt.x, pivot), bd = scaled(wt.x, table[2 * (size_t)b.x + 1]);
    if (b.y >= 0) {
        blendSlot(table, b.y, wt.y, pivot, br, bd);
        if (b.z >= 0) {
            blendSlot(table, b.z, wt.z, pivot, br, bd);
            if (b.w >= 0) blendSlot(table, b.w, wt.w, pivot, br, bd);
        }
    }
    const float L = sqrtf(((br.x * br.x + br.y * br.y) + br.z * br.z) + br.w * br.w);
    const float w = br.x / L, x = br.y / L, y = br.z / L, z = br.w / L;
    const float dw = bd.x / L, dx = bd.y / L, dy = bd.z / L, dz = bd.w / L;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    const float r00 = 1.0f - 2.0f * (yy + zz), r01 = 2.0f * (xy - wz), r02 = 2.0f * (xz + wy);
    const float r10 = 2.0f * (xy + wz), r11 = 1.0f - 2.0f * (xx + zz), r12 = 2.0f * (yz - wx);
    const float r20 = 2.0f * (xz - wy), r21 = 2.0f * (yz + wx), r22 = 1.0f - 2.0f * (xx + yy);
    const float t0 = 2.0f * (((dx * w - dw * x) + dz * y) - dy * z);
    const float t1 = 2.0f * (((dy * w - dw * y) + dx * z) - dz * x);
    const float t2 = 2.0f * (((dz * w - dw * z) + dy * x) - dx * y);
    const size_t at = 10 * (size_t)tri + c;
    const float4 v = rest[at], n = rest[at + 3];
    // pt_pose.hip's arithmetic, on the record with M = [R | t] and N = R
    out[at] = posePoint(make_float4(r00, r01, r02, t0), make_float4(r10, r11, r12, t1), make_float4(r20, r21, r22, t2), v);
    out[at + 3] = poseNormal(make_float4(r00, r01, r02, r10), make_float4(r11, r12, r20, r21), r22, n);
}

}  // namespace

hipError_t ptSkinDqRecordsLaunch(const float* xforms, int nParts, float* table, hipStream_t s) {
    if (nParts <= 0) return hipGetLastError();
    unsigned blocks;
    if (!gridOf(nParts, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dq_records, dim3(blocks), dim3(BLOCK), 0, s, reinterpret_cast<const float4*>(xforms), nParts, reinterpret_cast<float4*>(table));
    return hipGetLastError();
}

hipError_t ptSkinDqLaunch(const float* rest, const int32_t* bone, const float* weight, int64_t nTris, const float* table, float* out, hipStream_t s) {
    if (nTris <= 0) return hipGetLastError();
    const long long n = 3 * (long long)nTris;
    unsigned blocks;
    if (!gridOf(n, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_skin_dq_corners, dim3(blocks), dim3(BLOCK), 0, s, reinterpret_cast<const float4*>(rest), reinterpret_cast<const int4*>(bone),
                       reinterpret_cast<const float4*>(weight), n, reinterpret_cast<const float4*>(table), reinterpret_cast<float4*>(out));
    return hipGetLastError();
}
