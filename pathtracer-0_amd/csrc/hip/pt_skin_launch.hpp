// pt_skin_launch.hpp — the launch interface of the kernels of pt_skin.hip (include/pt_skin.h), called by the host half of the pose,
// pt_pose_host.hpp.  Every pointer is device memory; the launch is asynchronous on the given stream and returns hipGetLastError().
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// which statement of the skin rule runs: one lane per float4 (six per triangle), or one lane per corner (three per triangle).  Both give the same
// bits; the choice is a measurement's (scripts/skin_probe.py)
enum PtSkinKernel { PT_SKIN_PER_QUAD = 0, PT_SKIN_PER_CORNER = 1 };

// out (40 floats per triangle) gets the posed vertex and normal float4 of every corner whose slot 0 holds a bone; the rest of out, and the static
// corners, are not written: the caller filled them with the rest pose once.  bone / weight: 12 words per triangle, a corner's four at
// 12*k + 4*c, both 16-byte aligned.  xforms: 24 floats per bone, 16-byte aligned.
hipError_t ptSkinLaunch(const float* rest, const int32_t* bone, const float* weight, int64_t nTris, const float* xforms, float* out, PtSkinKernel which, hipStream_t s);
