// pt_move_launch.hpp — the launch interface of the kernels of pt_move.hip (include/pt_move.h), called by the host half of the in-place move,
// pt_move_host.hpp.  Every pointer is device memory; every launch is asynchronous on the given stream and returns hipGetLastError().
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct PtMovePatch {
    const float* tris;              // the new binding 3 (a plan's device copy), 40 floats per triangle
    const float* data;              // the refit binding 10 (a plan's working copy), 8 floats per node
    const int32_t* child;           // 2 node ids per inner record, in the layout's order (ptl::MoveMap::child)
    float4* triRecs; int nTriRecs;  // 48-byte triangle records
    float4* shade; int nTris;       // 64-byte shading records by triangle id
    float4* nodes; float* nodes80; int nInner, stride;      // 64-byte node records; the hand-written kernel's records of `stride` (80 or 64) bytes
    int* flag;                      // one int, zeroed by the launch: set when a node box it wrote has min > max or a NaN
};

// flag (one int, zeroed by the launch) is set when a triangle that a record references has a material index outside [0, nMat)
hipError_t ptMoveCheckLaunch(const float4* triRecs, int nTriRecs, const float* tris, int nMat, int* flag, hipStream_t s);
hipError_t ptMovePatchLaunch(const PtMovePatch& p, hipStream_t s);
