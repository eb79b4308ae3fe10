// pt_rig_ik_launch.hpp — the launch interface of the kernel of pt_rig_ik.hip (include/pt_rig_ik.h), called by the host half of the rig,
// pt_rig_host.hpp.  Every pointer is device memory, 16-byte aligned; the launch is asynchronous on the given stream and returns
// hipGetLastError().  It goes to the pose's stream between the levels that make the first joints' parents' world matrices and the levels that
// run over the changed locals: the kernel boundaries are the only ordering.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// rows: 16 bytes per constraint, ptp::RigIkRow (first's parent or -1, root, mid, tip | parent, joint, -1, -1); constraints and goals: 32 bytes
// per constraint each, as include/pt_rig_ik.h lays them out; world: 12 floats per joint.  Steps 0-7 of the rule, one lane per constraint: the
// locals are read at `in` and the written joints' quaternions stored at `out` (12 floats per joint each; the two may be the same array, and are
// in every call of the rig: the constraints are independent, so no lane reads what another writes)
hipError_t ptRigIkLaunch(const int32_t* rows, const void* constraints, const void* goals, int nConstraints, const float* world, const float* in, float* out, hipStream_t s);
