// pt_pose_launch.hpp — the launch interface of the kernels of pt_pose.hip (include/pt_pose.h), called by the host half of the pose,
// pt_pose_host.hpp.  Every pointer is device memory; every launch is asynchronous on the given stream and returns hipGetLastError().
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// which statement of k_pose runs: one lane per float4 (six per triangle), or one lane per triangle.  Both give the same bits; the choice is a
// measurement's (scripts/pose_probe.py)
enum PtPoseKernel { PT_POSE_PER_QUAD = 0, PT_POSE_PER_TRIANGLE = 1 };

// out (40 floats per triangle) gets the posed six leading float4 of every triangle whose part id is >= 0; the rest of out, and the triangles of
// part -1, are not written: the caller filled them with the rest pose once.  xforms: 24 floats per part, 16-byte aligned.
hipError_t ptPoseLaunch(const float* rest, const int32_t* triPart, int64_t nTris, const float* xforms, float* out, PtPoseKernel which, hipStream_t s);

// out row r (8 floats) = row ids[r] of data (binding 10); n rows
hipError_t ptPoseGatherLaunch(const float* data, const int32_t* ids, int n, float* out, hipStream_t s);

// motionPack's triangle records (pt_motion_pack.hpp) from a device binding 3: per triangle (A, flag), (B, 0), (C, 0).  then == nullptr: flag 0; else
// flag = 0 iff t < nThen and all nine floats compare equal to then's record t (a NaN never does), 1 otherwise
hipError_t ptPoseMotionLaunch(const float* tris, int nTris, const float4* then, int nThen, float4* out, hipStream_t s);
