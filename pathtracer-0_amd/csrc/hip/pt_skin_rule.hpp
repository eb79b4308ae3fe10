// pt_skin_rule.hpp — the host-only part of include/pt_skin.h: what pt_skin_create refuses in its arguments before its first HIP call (the first
// failing check as a code and one text each, in the header's order, each check over the whole table before the next), and a plain C++ statement
// of the rule that k_skin_quads and k_skin_corners (pt_skin.hip) are the device statements of.  Built on ptp::poseQuad: the blended record takes
// the place of the part's.  Plain C++: no HIP runtime call and no context, so tests/c/skin_rule_check.cpp runs all of it on a CPU.
#pragma once
#include "../../../include/pt_skin.h"
#include "pt_pose_rule.hpp"

#include <cmath>

namespace ptp {

// every check of pt_skin_create, in the order the header lists them
enum SkinCheck { SK_OK, SK_NULL, SK_BONE_BYTES, SK_WEIGHT_BYTES, SK_N_PARTS, SK_BONE_ID, SK_BONE_ORDER, SK_WEIGHT, SK_COUNT };

// nTris: the triangles of the context's binding 3 (read only once ctx is known not to be null); who: the entry point that answers
// (pt_skin_dq_create of include/pt_skin_dq.h takes the same tables and refuses the same)
inline Refused checkSkinCreate(const void* ctx, const int32_t* bone, size_t boneBytes, const float* weight, size_t weightBytes, int nParts, const void* out, size_t nTris,
                               int* which = nullptr, const char* who = "pt_skin_create") {
    auto refuse = [&](SkinCheck k, const char* text) {
        if (which) *which = k;
        return Refused{PT_ERR_ARG, std::string(who) + ": " + text};
    };
    if (which) *which = SK_OK;
    if (!ctx || !bone || !weight || !out) return refuse(SK_NULL, "null ctx, corner_bone, corner_weight or out");
    if (boneBytes != nTris * 48) return refuse(SK_BONE_BYTES, "bone_bytes != n_tris * 48");
    if (weightBytes != nTris * 48) return refuse(SK_WEIGHT_BYTES, "weight_bytes != n_tris * 48");
    if (nParts < 0 || nParts > PT_POSE_MAX_PARTS) return refuse(SK_N_PARTS, "n_parts must lie in 0 .. 65536");
    const size_t n = nTris * 12;
    for (size_t i = 0; i < n; i++)
        if (bone[i] < -1 || bone[i] >= nParts) return refuse(SK_BONE_ID, "a bone id outside [-1, n_parts)");
    for (size_t i = 0; i < n; i++)
        if ((i & 3) && bone[i] >= 0 && bone[i - 1] < 0) return refuse(SK_BONE_ORDER, "a bone id after an empty slot");
    for (size_t i = 0; i < n; i++)
        if (bone[i] >= 0 && !std::isfinite(weight[i])) return refuse(SK_WEIGHT, "a weight of a used slot that is not finite");
    return {};
}

// THE BLEND of one corner: B (24 floats; 21-23 zero) from the corner's four slots.  At least slot 0 is used.  Every product is rounded before
// every sum, in slot order.
inline void skinBlend(const int32_t* b, const float* w, const float* xforms, float* B) {
    const float* X = xforms + (size_t)PT_POSE_RECORD_FLOATS * (size_t)b[0];
    for (int j = 0; j < 21; j++) B[j] = w[0] * X[j];
    B[21] = B[22] = B[23] = 0.0f;
    for (int s = 1; s < PT_SKIN_SLOTS && b[s] >= 0; s++) {
        X = xforms + (size_t)PT_POSE_RECORD_FLOATS * (size_t)b[s];
        for (int j = 0; j < 21; j++) {
            const float p = w[s] * X[j];
            B[j] = B[j] + p;
        }
    }
}

// out (40 floats per triangle) = the rule applied to rest under the two tables and the pose's records; the tables were checked by checkSkinCreate
inline void skinTriangles(const float* rest, const int32_t* bone, const float* weight, size_t nTris, const float* xforms, float* out) {
    float B[PT_POSE_RECORD_FLOATS];
    for (size_t k = 0; k < nTris; k++) {
        const float* T = rest + 40 * k; float* O = out + 40 * k;
        for (int f = 0; f < 40; f++) O[f] = T[f];
        for (int c = 0; c < 3; c++) {
            const int32_t* b = bone + 12 * k + 4 * c;
            if (b[0] < 0) continue;
            skinBlend(b, weight + 12 * k + 4 * c, xforms, B);
            poseQuad(B, c, T + 4 * c, O + 4 * c);
            poseQuad(B, 3 + c, T + 12 + 4 * c, O + 12 + 4 * c);
        }
    }
}

}  // namespace ptp
