// pt_morph.hip — the kernel of include/pt_morph.h: the device statement of ptp::morphTriangles (pt_morph_rule.hpp), which is its specification.
// A scene-build file like pt_pose.hip and pt_skin.hip: no render kernel is here.
//
//   k_morph_corners  one lane per AFFECTED corner.  Its corner id and its row's bounds; the corner's vertex float4 and normal float4 from the rest
//                    pose; its row of entries in (corner, target) order, each entry two 16-byte loads and one weight from the table of at most
//                    1024 floats (4 KB: the caches serve it); two 16-byte stores into the morphed rest pose.  The row is walked four entries
//                    a step with no branch inside the step: the first statement, one entry a step behind `if (w == 0) continue`, was compiled
//                    into three dependent round trips per entry (target, weight, deltas) and ran at half this one's rate
// An inverted-index sum: per destination a list in a fixed order, so the bits do not depend on the launch.  A wave runs as long as its longest
// row; rows are not split, because the rule fixes the order of the sum (scripts/morph_probe.py measures a skewed table).  An entry whose weight
// compares equal to zero is skipped (loaded, not added): with every weight +-0 a corner's floats are stored as they were loaded.  Every lane writes its own two float4s
// and reads only what the host uploaded: kernel boundaries are the only ordering.  The file is compiled with -ffp-contract=off like the rest of
// the library, so v + w * d is a rounded product and a rounded sum.  Corner ids and targets were range-checked on the host (checkMorphAttach).
#include <hip/hip_runtime.h>

#include "pt_geom_steps.hpp"
#include "pt_morph_launch.hpp"

namespace {

// THE RULE, one entry: skipped when its weight compares equal to zero (or when `there` says the row has ended); every product rounded before
// every sum.  Selects, no branch: behind a branch the compiler moves the entry's loads, and the row becomes a chain of round trips
__device__ __forceinline__ void morphAdd(float4& v, float4& n, const bool there, const float w, const float4 a, const float4 b) {
    const bool on = there && w != 0.0f;
    v.x = on ? v.x + w * a.y : v.x; v.y = on ? v.y + w * a.z : v.y; v.z = on ? v.z + w * a.w : v.z;
    n.x = on ? n.x + w * b.x : n.x; n.y = on ? n.y + w * b.y : n.y; n.z = on ? n.z + w * b.z : n.z;
}

__global__ void __launch_bounds__(BLOCK) k_morph_corners(const float4* __restrict__ rest, const int* __restrict__ corner, const int* __restrict__ rowStart,
                                                        const float4* __restrict__ entries, const float* __restrict__ weights, long long nAffected,
                                                        float4* __restrict__ out) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nAffected) return;
    const int q = corner[i];
    const int first = rowStart[i], end = rowStart[i + 1];
    const int t = q / 3;
    const size_t at = 10 * (size_t)t + (size_t)(q - 3 * t);
    float4 v = rest[at], n = rest[at + 3];
    // four entries a step, in the row's order: the loads of all of them, then their weights, are in flight before the first sum.  An entry is
    // a = (target, dx, dy, dz), b = (dnx, dny, dnz, pad); where the row has ended its last entry is loaded again (no branch between the loads:
    // every index stays inside the row) and is not applied again
    for (int j = first; j < end; j += 4) {
        const int m = end - j;
        const float4* e = entries + 2 * (size_t)j;
        const int i1 = m > 1 ? 2 : 0, i2 = m > 2 ? 4 : i1, i3 = m > 3 ? 6 : i2;
        const float4 a0 = e[0], b0 = e[1], a1 = e[i1], b1 = e[i1 + 1], a2 = e[i2], b2 = e[i2 + 1], a3 = e[i3], b3 = e[i3 + 1];
        const float w0 = weights[__float_as_int(a0.x)], w1 = weights[__float_as_int(a1.x)], w2 = weights[__float_as_int(a2.x)], w3 = weights[__float_as_int(a3.x)];
        morphAdd(v, n, true, w0, a0, b0);
        morphAdd(v, n, m > 1, w1, a1, b1);
        morphAdd(v, n, m > 2, w2, a2, b2);
        morphAdd(v, n, m > 3, w3, a3, b3);
    }
    out[at] = v;
    out[at + 3] = n;
}

}  // namespace

hipError_t ptMorphLaunch(const float* rest, const int32_t* corner, const int32_t* rowStart, const void* entries, const float* weights, int64_t nAffected, float* out,
                         hipStream_t s) {
    if (nAffected <= 0) return hipGetLastError();
    unsigned blocks;
    if (!gridOf(nAffected, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_morph_corners, dim3(blocks), dim3(BLOCK), 0, s, reinterpret_cast<const float4*>(rest), corner, rowStart,
                       reinterpret_cast<const float4*>(entries), weights, (long long)nAffected, reinterpret_cast<float4*>(out));
    return hipGetLastError();
}
