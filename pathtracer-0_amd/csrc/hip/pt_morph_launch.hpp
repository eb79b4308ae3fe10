// pt_morph_launch.hpp — the launch interface of the kernel of pt_morph.hip (include/pt_morph.h), called by the host half of the pose,
// pt_pose_host.hpp.  Every pointer is device memory; the launch is asynchronous on the given stream and returns hipGetLastError().
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// out (40 floats per triangle) gets the morphed vertex and normal float4 of every AFFECTED corner — the nAffected corners of `corner`, ascending,
// each in [0, 3 * n_tris) — and nothing else: the caller filled out with the rest pose once.  rowStart: nAffected + 1 offsets into entries;
// entries: ptp::MorphEntry (pt_morph_rule.hpp), 32 bytes each, sorted by (corner, target), 16-byte aligned, every target below the length of
// weights.  rest and out: 16-byte aligned.  A grid above 0x7fffffff blocks is refused with hipErrorInvalidValue.
hipError_t ptMorphLaunch(const float* rest, const int32_t* corner, const int32_t* rowStart, const void* entries, const float* weights, int64_t nAffected, float* out,
                         hipStream_t s);
