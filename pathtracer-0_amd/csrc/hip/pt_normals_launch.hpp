// pt_normals_launch.hpp — the launch interface of the kernels of pt_normals.hip (include/pt_normals.h), called by the host half of the pose,
// pt_pose_host.hpp.  Every pointer is device memory; the launches are asynchronous on the given stream and return hipGetLastError().
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// the two statements of the gather: the same bits by construction (pt_debug_normals_time runs either)
enum PtNormalsKernel { PT_NORMALS_PER_VERTEX = 0, PT_NORMALS_PER_CORNER = 1 };

// faces (4 floats per triangle, 16-byte aligned, indexed by triangle id) gets the face vector of each of the nListed triangles of `tris`
// (ascending ids in [0, n_tris)) from the vertices of dst (40 floats per triangle, 16-byte aligned); flip: every component negated.  Nothing else
// of faces is written.  A grid above 0x7fffffff blocks is refused with hipErrorInvalidValue.
hipError_t ptNormalsFacesLaunch(const float* dst, const int32_t* tris, int64_t nListed, int flip, float* faces, hipStream_t s);

// The normals of dst's corners listed in `corners` (nEntries corners with an id >= 0, sorted by (id, corner), each in [0, 3 * n_tris)) from
// faces: rowStart holds nRows + 1 offsets into corners, one row per non-empty vertex; cornerRow per entry its row.  A row whose length is not
// finite and > 0 is left as it is.  Only floats 12+4c .. 12+4c+2 of the listed corners are written.  A grid above 0x7fffffff blocks is refused.
hipError_t ptNormalsGatherLaunch(const float* faces, const int32_t* rowStart, int64_t nRows, const int32_t* corners, const int32_t* cornerRow, int64_t nEntries,
                                 float* dst, PtNormalsKernel which, hipStream_t s);
