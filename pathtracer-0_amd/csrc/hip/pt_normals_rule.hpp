// pt_normals_rule.hpp — the host-only part of include/pt_normals.h: what pt_normals_attach and pt_normals_mode refuse in their arguments (the
// first failing check as a code and one text each, in the header's order, each check over the whole table before the next), the inverted index
// that the kernels of pt_normals.hip read, and a plain C++ statement of the rule that those kernels are the device statement of.  Plain C++: no
// HIP runtime call and no context, so tests/c/normals_rule_check.cpp runs all of it on a CPU.  Whether a pose is live, whether it has normals and
// which of its corners its rule moves are the host half's to say (pt_pose_host.hpp); they arrive here as answers.
#pragma once
#include "../../../include/pt_normals.h"
#include "pt_pose_rule.hpp"

#include <cmath>
#include <vector>

namespace ptp {

// every check of pt_normals_attach, in the order the header lists them, then those of pt_normals_mode
enum NormalsCheck { NC_OK, NC_NULL, NC_ATTACHED, NC_FLAGS, NC_N_VERTICES, NC_VERTEX_BYTES, NC_ID, NC_TWICE, NC_STATIC, NM_POSE, NM_NO_NORMALS, NM_ON, NC_COUNT };

// live: the pose is neither null nor destroyed; hasNormals, nTris and moved (one byte per corner, 3 * nTris: non-zero where the pose's rule writes
// the corner) are read only when live
inline Refused checkNormalsAttach(bool live, bool hasNormals, const int32_t* cornerVertex, size_t vertexBytes, int64_t nVertices, uint32_t flags, size_t nTris,
                                  const unsigned char* moved, int* which = nullptr) {
    auto no = [&](NormalsCheck k, const char* text) {
        if (which) *which = k;
        return Refused{PT_ERR_ARG, std::string("pt_normals_attach: ") + text};
    };
    if (which) *which = NC_OK;
    if (!live || !cornerVertex) return no(NC_NULL, "null or destroyed pose, or null corner_vertex");
    if (hasNormals) return no(NC_ATTACHED, "the pose has normals attached already");
    if (flags & ~(uint32_t)PT_NORMALS_FLIP) return no(NC_FLAGS, "a bit of flags other than PT_NORMALS_FLIP");
    if (nVertices < 0 || (uint64_t)nVertices > 3 * (uint64_t)nTris) return no(NC_N_VERTICES, "n_vertices outside [0, 3 * n_tris]");
    if (vertexBytes != nTris * 12) return no(NC_VERTEX_BYTES, "vertex_bytes != n_tris * 12");
    const size_t nCorners = 3 * nTris;
    for (size_t q = 0; q < nCorners; q++)
        if (cornerVertex[q] < -1 || cornerVertex[q] >= nVertices) return no(NC_ID, "an id outside [-1, n_vertices)");
    for (size_t k = 0; k < nTris; k++) {
        const int32_t a = cornerVertex[3 * k], b = cornerVertex[3 * k + 1], c = cornerVertex[3 * k + 2];
        if ((a >= 0 && (a == b || a == c)) || (b >= 0 && b == c)) return no(NC_TWICE, "the same id >= 0 at two corners of one triangle");
    }
    for (size_t q = 0; q < nCorners; q++)
        if (cornerVertex[q] >= 0 && !moved[q]) return no(NC_STATIC, "an id >= 0 at a corner that the pose's rule leaves static");
    return {};
}

inline Refused checkNormalsMode(bool live, bool hasNormals, int on, int* which = nullptr) {
    auto no = [&](NormalsCheck k, const char* text) {
        if (which) *which = k;
        return Refused{PT_ERR_ARG, std::string("pt_normals_mode: ") + text};
    };
    if (which) *which = NC_OK;
    if (!live) return no(NM_POSE, "null or destroyed pose");
    if (!hasNormals) return no(NM_NO_NORMALS, "the pose has no normals attached");
    if (on != 0 && on != 1) return no(NM_ON, "on must be 0 or 1");
    return {};
}

// THE INVERTED INDEX of a checked table.  tris: the triangles with at least one id >= 0, ascending.  verts: the ids that some corner names,
// ascending, one row each (rowStart: verts.size() + 1 offsets into corners).  corners: every corner with an id >= 0 exactly once, by (id, corner)
// — a stable counting sort over the corners in ascending order, which is the order of the rule's sum.  cornerRow: per entry of corners the index
// of its row (what the per-corner statement of the gather starts from).
struct NormalRows {
    std::vector<int32_t> tris, verts, rowStart, corners, cornerRow;
};
inline void normalRows(const int32_t* cornerVertex, size_t nTris, int64_t nVertices, NormalRows& out) {
    const size_t nCorners = 3 * nTris;
    std::vector<int32_t> at((size_t)nVertices, 0), rowOf((size_t)nVertices, -1);      // first the count per id, then the cursor of its row
    out.tris.clear(); out.verts.clear(); out.rowStart.clear();
    size_t named = 0;
    for (size_t k = 0; k < nTris; k++) {
        bool any = false;
        for (int c = 0; c < 3; c++)
            if (cornerVertex[3 * k + c] >= 0) { at[(size_t)cornerVertex[3 * k + c]]++; named++; any = true; }
        if (any) out.tris.push_back((int32_t)k);
    }
    int32_t sum = 0;
    for (size_t g = 0; g < (size_t)nVertices; g++) {
        if (!at[g]) continue;
        rowOf[g] = (int32_t)out.verts.size();
        out.verts.push_back((int32_t)g);
        out.rowStart.push_back(sum);
        const int32_t n = at[g];
        at[g] = sum;
        sum += n;
    }
    out.rowStart.push_back(sum);
    out.corners.assign(named, 0); out.cornerRow.assign(named, 0);
    for (size_t q = 0; q < nCorners; q++) {
        const int32_t g = cornerVertex[q];
        if (g < 0) continue;
        const size_t e = (size_t)at[(size_t)g]++;
        out.corners[e] = (int32_t)q;
        out.cornerRow[e] = rowOf[(size_t)g];
    }
}

// THE RULE, step 1: the face vector of one triangle (40 floats) into F[3]; every product rounded before every difference
inline void normalsFace(const float* t, bool flip, float* F) {
    const float e1x = t[4] - t[0], e1y = t[5] - t[1], e1z = t[6] - t[2];
    const float e2x = t[8] - t[0], e2y = t[9] - t[1], e2z = t[10] - t[2];
    const float a = e1y * e2z, b = e1z * e2y, c = e1z * e2x, d = e1x * e2z, e = e1x * e2y, f = e1y * e2x;
    F[0] = a - b; F[1] = c - d; F[2] = e - f;
    if (flip) { F[0] = -F[0]; F[1] = -F[1]; F[2] = -F[2]; }
}

// steps 2-4 for one row: the sum in the row's order, the length, the divide.  false: the fallback (nothing is to be stored)
inline bool normalsOfRow(const float* faces, const int32_t* row, int32_t n, float* N) {
    float S[3];
    for (int j = 0; j < 3; j++) S[j] = faces[4 * (size_t)(row[0] / 3) + j];
    for (int32_t i = 1; i < n; i++)
        for (int j = 0; j < 3; j++) S[j] = S[j] + faces[4 * (size_t)(row[i] / 3) + j];
    const float xx = S[0] * S[0], yy = S[1] * S[1], zz = S[2] * S[2];
    const float s2 = xx + yy;
    const float L = std::sqrt(s2 + zz);
    if (!(std::isfinite(L) && L > 0.0f)) return false;
    for (int j = 0; j < 3; j++) N[j] = S[j] / L;
    return true;
}

// tris (40 floats per triangle, in place): the pose's rule has written it; the rule over a whole binding 3.  -> the number of rows that took the fallback
inline size_t smoothNormals(float* tris, size_t nTris, const NormalRows& rows, uint32_t flags) {
    std::vector<float> faces(4 * nTris, 0.0f);
    for (const int32_t k : rows.tris) normalsFace(tris + 40 * (size_t)k, (flags & PT_NORMALS_FLIP) != 0, faces.data() + 4 * (size_t)k);
    size_t fell = 0;
    for (size_t i = 0; i < rows.verts.size(); i++) {
        const int32_t* row = rows.corners.data() + rows.rowStart[i];
        const int32_t n = rows.rowStart[i + 1] - rows.rowStart[i];
        float N[3];
        if (!normalsOfRow(faces.data(), row, n, N)) { fell++; continue; }
        for (int32_t e = 0; e < n; e++) {
            const size_t q = (size_t)row[e], k = q / 3, c = q - 3 * k;
            for (int j = 0; j < 3; j++) tris[40 * k + 12 + 4 * c + j] = N[j];
        }
    }
    return fell;
}

}  // namespace ptp
