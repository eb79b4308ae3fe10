// pt_refit_state.hpp — what a refit plan (include/pt_refit.h) holds on its device, shared by pt_refit.hip, which owns it, and the in-place move
// (include/pt_move.h: pt_move.hip and its host half pt_move_host.hpp), which reads the plan's binding 3 and refit binding 10 where a run left them.
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/pt_refit.h"
#include "pt_devmem.hpp"
#include "pt_refit_plan.hpp"
#include "pt_scene_move.hpp"

struct pt_refit_plan {
    int device = 0;
    ptr::RefitSchedule s;                                // (host copy: the launch sizes, the roots)
    size_t dataBytes = 0; int64_t nTris = 0;
    uint64_t digest = 0;                                 // ptr::topologyDigest of the buffers it was made from
    hipStream_t stream = nullptr;
    Dev<float> dData;                                    // binding 10 as created; every run rewrites floats 0-5 of the reachable rows
    Dev<float> dTris;                                    // binding 3 of the current run
    Dev<int32_t> dTree, dLeaf, dOrder, dLevelStart, dRoots;
    Dev<double> dS, dRootCost;
    Dev<int> dFlag;
    // pt_move_geometry: the map of the layout order (pt_scene_move.hpp) for the bfs_nodes it was made under, on the host and, the children of
    // every inner record, on the device.  Made by the first call; a plan that never moves a context holds none.
    ptl::MoveMap map; bool mapValid = false; int mapBfsNodes = 0; Dev<int32_t> dMapChild;
    ~pt_refit_plan() {
        if (!stream) return;                             // refused before anything was allocated
        // the device memory goes before the stream, on the plan's device
        hipSetDevice(device);
        dData.release(); dTris.release(); dTree.release(); dLeaf.release(); dOrder.release(); dLevelStart.release(); dRoots.release();
        dS.release(); dRootCost.release(); dFlag.release(); dMapChild.release();
        if (stream) hipStreamDestroy(stream);
    }
};

// pt_refit.hip.  Whether the plan is live (a destroyed one is refused, not followed), and the device half of a run: the upload of binding 3, the
// kernels, the NaN flag read back; the plan's stream is idle afterwards and dData / dRootCost hold the result.  PT_OK, PT_ERR_SCENE for a NaN
// (`who` heads the text), PT_ERR_HIP.
bool pt_refit_live_(pt_refit_plan* plan);
int pt_refit_device_(pt_refit_plan* plan, const float* tris, size_t tri_bytes, const char* who);
// ... and its second half alone, for a caller whose kernels have left binding 3 in plan->dTris on the plan's stream (include/pt_pose.h)
int pt_refit_kernels_(pt_refit_plan* plan, const char* who);
