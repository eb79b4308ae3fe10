// pt_rig_mix_launch.hpp — the launch interface of the kernel of pt_rig_mix.hip (include/pt_rig_mix.h), called by the host half of the rig,
// pt_rig_host.hpp.  Every pointer is device memory, 16-byte aligned (a mask: 4-byte); the launch is asynchronous on the given stream and returns
// hipGetLastError().  It goes to the pose's stream ahead of the rig's levels: the kernel boundary between them is the only ordering.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int PT_RIG_MIX_TABLE_LAYERS = 8;      // PT_RIG_MIX_MAX_LAYERS of include/pt_rig_mix.h

// the layer table, by value in the kernel arguments: uniform over the launch.  Per layer the locals of keys ka, kb and 0 of its slot (12 floats
// per joint), its mask (one float per joint) or null, u (0: key ka alone, kb is not read), weight and mode (0 override, 1 additive; the
// first layer is the base whatever it says)
struct PtRigMixTable {
    const float* a[PT_RIG_MIX_TABLE_LAYERS];
    const float* b[PT_RIG_MIX_TABLE_LAYERS];
    const float* r[PT_RIG_MIX_TABLE_LAYERS];
    const float* mask[PT_RIG_MIX_TABLE_LAYERS];
    float u[PT_RIG_MIX_TABLE_LAYERS], weight[PT_RIG_MIX_TABLE_LAYERS];
    int32_t mode[PT_RIG_MIX_TABLE_LAYERS];
    int32_t nLayers;                             // 1 .. PT_RIG_MIX_TABLE_LAYERS
};

// out (12 floats per joint, paddings 0) = steps 2-7 of the rule over the table's layers, one lane per joint
hipError_t ptRigMixLaunch(const PtRigMixTable& table, int nJoints, float* out, hipStream_t s);
