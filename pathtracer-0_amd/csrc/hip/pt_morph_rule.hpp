// pt_morph_rule.hpp — the host-only part of include/pt_morph.h: what pt_morph_attach and pt_morph_weights refuse in their arguments (the first
// failing check as a code and one text each, in the header's order, each check over the whole table before the next), the inverted index that
// k_morph_corners (pt_morph.hip) reads, and a plain C++ statement of the rule that the kernel is the device statement of.  Plain C++: no HIP
// runtime call and no context, so tests/c/morph_rule_check.cpp runs all of it on a CPU.  Whether a pose is live, whether it has a morph and which
// of its corners its rule moves are the host half's to say (pt_pose_host.hpp); they arrive here as answers.
#pragma once
#include "../../../include/pt_morph.h"
#include "pt_pose_rule.hpp"

#include <cmath>
#include <vector>

namespace ptp {

// every check of pt_morph_attach, in the order the header lists them, then those of pt_morph_weights
enum MorphCheck { MC_OK, MC_NULL, MC_ATTACHED, MC_N_TARGETS, MC_START_BYTES, MC_STARTS, MC_CORNER_BYTES, MC_DELTA_BYTES, MC_CORNER, MC_TWICE, MC_DELTA, MC_STATIC,
                  MW_POSE, MW_NO_MORPH, MW_NULL, MW_BYTES, MW_WEIGHT, MC_COUNT };

// one entry as the kernel loads it: two aligned 16-byte loads
struct MorphEntry { int32_t target; float d[6]; int32_t pad; };
static_assert(sizeof(MorphEntry) == 32, "an entry is two float4");

// live: the pose is neither null nor destroyed; hasMorph, nTris and moved (one byte per corner, 3 * nTris: non-zero where the pose's rule writes the
// corner) are read only when live
inline Refused checkMorphAttach(bool live, bool hasMorph, int nTargets, const int64_t* targetStart, size_t startBytes, const int32_t* entryCorner, size_t cornerBytes,
                                const float* entryDelta, size_t deltaBytes, size_t nTris, const unsigned char* moved, int* which = nullptr) {
    auto no = [&](MorphCheck k, const char* text) {
        if (which) *which = k;
        return Refused{PT_ERR_ARG, std::string("pt_morph_attach: ") + text};
    };
    if (which) *which = MC_OK;
    if (!live || !targetStart || !entryCorner || !entryDelta) return no(MC_NULL, "null or destroyed pose, or null target_start, entry_corner or entry_delta");
    if (hasMorph) return no(MC_ATTACHED, "the pose has a morph already");
    if (nTargets < 1 || nTargets > PT_MORPH_MAX_TARGETS) return no(MC_N_TARGETS, "n_targets must lie in 1 .. 1024");
    if (startBytes != ((size_t)nTargets + 1) * 8) return no(MC_START_BYTES, "start_bytes != (n_targets + 1) * 8");
    if (targetStart[0] != 0 || targetStart[nTargets] > 0x7fffffffLL) return no(MC_STARTS, "target_start is not 0 = s_0 <= s_1 <= ... <= s_n <= 0x7fffffff");
    for (int t = 0; t < nTargets; t++)
        if (targetStart[t] > targetStart[t + 1]) return no(MC_STARTS, "target_start is not 0 = s_0 <= s_1 <= ... <= s_n <= 0x7fffffff");
    const size_t E = (size_t)targetStart[nTargets];
    if (cornerBytes != E * 4) return no(MC_CORNER_BYTES, "corner_bytes != E * 4");
    if (deltaBytes != E * 24) return no(MC_DELTA_BYTES, "delta_bytes != E * 24");
    const size_t nCorners = 3 * nTris;
    for (size_t e = 0; e < E; e++)
        if (entryCorner[e] < 0 || (size_t)entryCorner[e] >= nCorners) return no(MC_CORNER, "a corner outside [0, 3 * n_tris)");
    {
        std::vector<int32_t> last(nCorners, -1);                  // the last target that named the corner
        for (int t = 0; t < nTargets; t++)
            for (size_t e = (size_t)targetStart[t]; e < (size_t)targetStart[t + 1]; e++) {
                int32_t& l = last[(size_t)entryCorner[e]];
                if (l == t) return no(MC_TWICE, "the same corner twice in one target");
                l = t;
            }
    }
    for (size_t e = 0; e < 6 * E; e++)
        if (!std::isfinite(entryDelta[e])) return no(MC_DELTA, "a delta that is not finite");
    for (size_t e = 0; e < E; e++)
        if (!moved[(size_t)entryCorner[e]]) return no(MC_STATIC, "a corner that the pose's rule leaves static");
    return {};
}

// nTargets: the morph's (read only when live and hasMorph)
inline Refused checkMorphWeights(bool live, bool hasMorph, const float* weights, size_t weightBytes, int nTargets, int* which = nullptr) {
    auto no = [&](MorphCheck k, const char* text) {
        if (which) *which = k;
        return Refused{PT_ERR_ARG, std::string("pt_morph_weights: ") + text};
    };
    if (which) *which = MC_OK;
    if (!live) return no(MW_POSE, "null or destroyed pose");
    if (!hasMorph) return no(MW_NO_MORPH, "the pose has no morph");
    if (!weights) return no(MW_NULL, "null weights");
    if (weightBytes != (size_t)nTargets * 4) return no(MW_BYTES, "weight_bytes != n_targets * 4");
    for (int t = 0; t < nTargets; t++)
        if (!std::isfinite(weights[t])) return no(MW_WEIGHT, "a weight that is not finite");
    return {};
}

// THE INVERTED INDEX of a checked table: the affected corners in ascending order, one row per affected corner (rowStart: corners.size() + 1
// offsets into entries), the entries sorted by (corner, target) — a stable counting sort over the targets in ascending order, which a corner
// named at most once per target makes the order of the rule.  nCorners = 3 * n_tris.
struct MorphRows {
    std::vector<int32_t> corners, rowStart;
    std::vector<MorphEntry> entries;
};
inline void morphRows(int nTargets, const int64_t* targetStart, const int32_t* entryCorner, const float* entryDelta, size_t nCorners, MorphRows& out) {
    const size_t E = (size_t)targetStart[nTargets];
    std::vector<int32_t> at(nCorners, 0);                         // first the count per corner, then the cursor of its row
    for (size_t e = 0; e < E; e++) at[(size_t)entryCorner[e]]++;
    out.corners.clear(); out.rowStart.clear();
    int32_t sum = 0;
    for (size_t q = 0; q < nCorners; q++) {
        if (!at[q]) continue;
        out.corners.push_back((int32_t)q);
        out.rowStart.push_back(sum);
        const int32_t n = at[q];
        at[q] = sum;
        sum += n;
    }
    out.rowStart.push_back(sum);
    out.entries.assign(E, MorphEntry{0, {0, 0, 0, 0, 0, 0}, 0});
    for (int t = 0; t < nTargets; t++)
        for (size_t e = (size_t)targetStart[t]; e < (size_t)targetStart[t + 1]; e++) {
            MorphEntry& m = out.entries[(size_t)at[(size_t)entryCorner[e]]++];
            m.target = t;
            for (int j = 0; j < 6; j++) m.d[j] = entryDelta[6 * e + j];
        }
}

// THE RULE, one affected corner: v (the vertex's float4) and n (the normal's) from the rest pose's, over the corner's row.  Every product is
// rounded before every sum; an entry whose weight compares equal to zero is skipped; the fourth floats are carried through.
inline void morphCorner(const MorphEntry* row, int32_t nEntries, const float* weights, float* v, float* n) {
    for (int32_t j = 0; j < nEntries; j++) {
        const float w = weights[row[j].target];
        if (w == 0.0f) continue;
        for (int i = 0; i < 3; i++) {
            const float p = w * row[j].d[i], pn = w * row[j].d[3 + i];
            v[i] = v[i] + p;
            n[i] = n[i] + pn;
        }
    }
}

// out (40 floats per triangle) = the morphed rest pose: the rule over a whole binding 3
inline void morphTriangles(const float* rest, size_t nTris, const MorphRows& rows, const float* weights, float* out) {
    for (size_t f = 0; f < 40 * nTris; f++) out[f] = rest[f];
    for (size_t i = 0; i < rows.corners.size(); i++) {
        const size_t q = (size_t)rows.corners[i], k = q / 3, c = q - 3 * k;
        morphCorner(rows.entries.data() + rows.rowStart[i], rows.rowStart[i + 1] - rows.rowStart[i], weights, out + 40 * k + 4 * c, out + 40 * k + 12 + 4 * c);
    }
}

}  // namespace ptp
