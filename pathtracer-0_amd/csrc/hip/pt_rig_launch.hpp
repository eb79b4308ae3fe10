// pt_rig_launch.hpp — the launch interface of the kernels of pt_rig.hip (include/pt_rig.h), called by the host half of the rig,
// pt_rig_host.hpp.  Every pointer is device memory, 16-byte aligned; a launch is asynchronous on the given stream and returns
// hipGetLastError().  The launches of one evaluation go to one stream, the blend (when there is one) first, then the levels from the roots
// down: the kernel boundaries between them are the only ordering.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// out (12 floats per joint) = the locals a and b of two keys under u (neither 0 nor 1), step 5 of the rule
hipError_t ptRigBlendLaunch(const float* a, const float* b, float u, int nJoints, float* out, hipStream_t s);

// steps 1-4 for the `count` joints order[first .. first + count) of one level: world (12 floats per joint) and records (24 floats per joint) are
// written at those joints' own ids; world is read at their parents', which an earlier launch wrote.  parent is indexed by joint id; invBind
// (12 floats per joint) may be null
hipError_t ptRigLevelLaunch(const int32_t* order, int first, int count, const int32_t* parent, const float* locals, const float* invBind, float* world, float* records,
                            hipStream_t s);
