// pt_skin_dq_launch.hpp — the launch interface of the kernels of pt_skin_dq.hip (include/pt_skin_dq.h), called by the host half of the pose,
// pt_pose_host.hpp.  Every pointer is device memory; a launch is asynchronous on the given stream and returns hipGetLastError().  The two launches
// go to one stream, the records first: the kernel boundary between them is the only ordering.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// table (8 floats per record: the real part, the dual part) from floats 0-11 of each of the nParts records of 24 floats; both 16-byte aligned
hipError_t ptSkinDqRecordsLaunch(const float* xforms, int nParts, float* table, hipStream_t s);

// out (40 floats per triangle) gets the posed vertex and normal float4 of every corner whose slot 0 holds a bone; the rest of out, and the static
// corners, are not written: the caller filled them with the rest pose once.  bone / weight: 12 words per triangle, a corner's four at
// 12*k + 4*c, both 16-byte aligned.  table: what ptSkinDqRecordsLaunch wrote.
hipError_t ptSkinDqLaunch(const float* rest, const int32_t* bone, const float* weight, int64_t nTris, const float* table, float* out, hipStream_t s);
