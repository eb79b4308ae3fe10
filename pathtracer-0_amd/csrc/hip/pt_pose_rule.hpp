// pt_pose_rule.hpp — the host-only part of include/pt_pose.h: what pt_pose_create, pt_pose_geometry and pt_pose_triangles refuse in their arguments
// before their first HIP call (the first failing check as a code and one text each, in the header's order), and a plain C++ statement of the rule
// that k_pose (pt_pose.hip) is the device statement of.  Plain C++: no HIP runtime call and no context, so tests/c/pose_rule_check.cpp runs all of
// it on a CPU.  Whether a pose is live and whose it is are the registry's to say (pt_pose_host.hpp); they arrive here as two answers.
#pragma once
#include "../../../include/pt_pose.h"
#include "pt_image_history.hpp"      // ptp::Refused

#include <cstddef>
#include <cstdint>
#include <string>

namespace ptp {

// every check below, in the order the header lists them (the test requires each of them of its grid)
enum PoseCheck { PC_OK, PC_NULL, PC_PART_BYTES, PC_N_PARTS, PC_PART_ID, PC_POSE, PC_FOREIGN, PC_XFORMS, PC_XFORM_BYTES, PC_ELLIP_BYTES, PC_TRIS_OUT, PC_TRI_BYTES, PC_COUNT };

namespace pose_detail {
inline Refused refuse(const char* who, int* which, PoseCheck k, const char* text) {
    if (which) *which = k;
    return Refused{PT_ERR_ARG, std::string(who) + ": " + text};
}
}  // namespace pose_detail

// pt_pose_create; nTris: the triangles of the context's binding 3 (read only once ctx is known not to be null)
inline Refused checkPoseCreate(const void* ctx, const int32_t* triPart, size_t partBytes, int nParts, const void* out, size_t nTris, int* which = nullptr) {
    using pose_detail::refuse;
    const char* who = "pt_pose_create";
    if (which) *which = PC_OK;
    if (!ctx || !triPart || !out) return refuse(who, which, PC_NULL, "null ctx, tri_part or out");
    if (partBytes != nTris * 4) return refuse(who, which, PC_PART_BYTES, "part_bytes != n_tris * 4");
    if (nParts < 0 || nParts > PT_POSE_MAX_PARTS) return refuse(who, which, PC_N_PARTS, "n_parts must lie in 0 .. 65536");
    for (size_t k = 0; k < nTris; k++)
        if (triPart[k] < -1 || triPart[k] >= nParts) return refuse(who, which, PC_PART_ID, "a part id outside [-1, n_parts)");
    return {};
}

// the matrices of a pose, for both calls that take them
inline Refused checkPoseXforms(const char* who, const float* xforms, size_t xformBytes, int nParts, int* which) {
    using pose_detail::refuse;
    if (!xforms && nParts > 0) return refuse(who, which, PC_XFORMS, "null xforms with n_parts > 0");
    if (xformBytes != (size_t)nParts * (PT_POSE_RECORD_FLOATS * 4)) return refuse(who, which, PC_XFORM_BYTES, "xform_bytes != n_parts * 96");
    return {};
}

// pt_pose_geometry; live: the pose is neither null nor destroyed; own: it was created on ctx; nParts: the pose's (read only when live)
inline Refused checkPoseGeometry(const void* ctx, bool live, bool own, const float* xforms, size_t xformBytes, int nParts, const float* ellip, size_t ellipBytes,
                                 int* which = nullptr) {
    using pose_detail::refuse;
    const char* who = "pt_pose_geometry";
    if (which) *which = PC_OK;
    if (!ctx) return refuse(who, which, PC_NULL, "null ctx");
    if (!live) return refuse(who, which, PC_POSE, "null or destroyed pose");
    if (!own) return refuse(who, which, PC_FOREIGN, "the pose was created on another context");
    if (Refused r = checkPoseXforms(who, xforms, xformBytes, nParts, which); r.code) return r;
    if (ellip && ellipBytes % 4) return refuse(who, which, PC_ELLIP_BYTES, "ellip_bytes must be a multiple of 4 bytes");
    return {};
}

// pt_pose_triangles
inline Refused checkPoseTriangles(bool live, const float* xforms, size_t xformBytes, int nParts, const float* trisOut, size_t triBytes, size_t nTris, int* which = nullptr) {
    using pose_detail::refuse;
    const char* who = "pt_pose_triangles";
    if (which) *which = PC_OK;
    if (!live) return refuse(who, which, PC_POSE, "null or destroyed pose");
    if (Refused r = checkPoseXforms(who, xforms, xformBytes, nParts, which); r.code) return r;
    if (!trisOut) return refuse(who, which, PC_TRIS_OUT, "null tris_out");
    if (triBytes != nTris * 160) return refuse(who, which, PC_TRI_BYTES, "tri_bytes != n_tris * 160");
    return {};
}

// THE RULE, one float4 of a triangle: q = 0, 1, 2 a vertex under M (floats 0-11 of the record), q = 3, 4, 5 a normal under N (floats 12-20); the
// fourth float is carried through.  Every product is rounded before every sum, in the written order.
inline void poseQuad(const float* X, int q, const float* in, float* out) {
    const float x = in[0], y = in[1], z = in[2];
    if (q < 3) {
        for (int i = 0; i < 3; i++) {
            const float* m = X + 4 * i;
            const float a = m[0] * x, b = m[1] * y, c = m[2] * z;
            out[i] = ((a + b) + c) + m[3];
        }
    } else {
        for (int i = 0; i < 3; i++) {
            const float* n = X + 12 + 3 * i;
            const float a = n[0] * x, b = n[1] * y, c = n[2] * z;
            out[i] = (a + b) + c;
        }
    }
    out[3] = in[3];
}

// out (40 floats per triangle) = the rule applied to rest under the part ids and the pose's records; part ids were checked by checkPoseCreate
inline void poseTriangles(const float* rest, const int32_t* triPart, size_t nTris, const float* xforms, float* out) {
    for (size_t k = 0; k < nTris; k++) {
        const float* T = rest + 40 * k; float* O = out + 40 * k;
        for (int f = 0; f < 40; f++) O[f] = T[f];
        if (triPart[k] < 0) continue;
        const float* X = xforms + (size_t)PT_POSE_RECORD_FLOATS * (size_t)triPart[k];
        for (int q = 0; q < 6; q++) poseQuad(X, q, T + 4 * q, O + 4 * q);
    }
}

}  // namespace ptp
