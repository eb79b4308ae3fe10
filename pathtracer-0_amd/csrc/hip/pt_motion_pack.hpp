// pt_motion_pack.hpp — where the primitives are, for include/pt_motion.h's mark and for the reprojection across moved geometry: the host copies of
// bindings 3 and 7 into plain positions, and those positions (against the mark's, when there is one) into the flagged records the kernel reads.
// Plain C++ over plain floats: no HIP runtime call and no context.  pt_image.hpp keeps the mark and uploads what this packs;
// tests/c/image_args_check.cpp packs small primitive lists on a CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

namespace ptp {

// the mark's host copies of the positions and their counts
struct MotionThen { const float* tri; int nTri; const float* el; int nEl; };

// the vertices of the triangles of binding 3 (9 floats each) and centre, stretch, rot, r of the ellipsoids of binding 7 (10 floats each), from the host copies
inline void motionPositions(const std::vector<float>& tris, const std::vector<float>& ellip, std::vector<float>& tri, int* nTri, std::vector<float>& el, int* nEl) {
    const size_t nt = tris.size() / 40;
    tri.resize(nt * 9);
    for (size_t t = 0; t < nt; t++)
        for (int v = 0; v < 3; v++) std::memcpy(&tri[9 * t + 3 * v], &tris[40 * t + 4 * v], 12);
    // the count as the scene build reads it: a NaN, a negative or a count beyond int is no ellipsoid here, and so is a buffer shorter than its
    // count says (buildScene refuses such a buffer)
    int ne = (!ellip.empty() && ellip[0] >= 0.0f && ellip[0] < 2147483648.0f) ? (int)ellip[0] : 0;
    if (ellip.size() < (size_t)1 + 11 * (size_t)ne) ne = 0;
    el.resize((size_t)ne * 10);
    const float* E = ellip.data();
    for (int i = 0; i < ne; i++) {
        for (int k = 0; k < 3; k++) { el[10 * i + k] = E[1 + 3 * i + k]; el[10 * i + 3 + k] = E[1 + ne * 3 + 3 * i + k]; el[10 * i + 6 + k] = E[1 + ne * 6 + 3 * i + k]; }
        el[10 * i + 9] = E[1 + ne * 9 + i];
    }
    *nTri = (int)nt; *nEl = ne;
}

// ... as the kernel reads them, twelve floats per primitive: triangle (A, flag), (B, 0), (C, 0); ellipsoid (c, r), (stretch, flag), (rot, 0); each array
// at least one zero 16-byte record.  then == nullptr: the mark's own copy, flags 0; else flag = 0 unmoved (every float compares equal), 1 moved (a
// NaN never compares equal; a primitive beyond the mark's count is moved), 2 a moved ellipsoid with a rot component != 0 then or now (-0.0 is 0)
inline void motionPack(const std::vector<float>& tri, int nTri, const std::vector<float>& el, int nEl, const MotionThen* then, std::vector<float>& outTri,
                       std::vector<float>& outEl) {
    auto asf = [](int u) { float f; std::memcpy(&f, &u, 4); return f; };
    outTri.assign(std::max<size_t>((size_t)nTri * 12, 4), 0.0f); outEl.assign(std::max<size_t>((size_t)nEl * 12, 4), 0.0f);
    for (int t = 0; t < nTri; t++) {
        const float* T = &tri[9 * (size_t)t];
        int flag = 0;
        if (then) {
            flag = t < then->nTri ? 0 : 1;
            for (int k = 0; k < 9 && !flag; k++) if (!(T[k] == then->tri[9 * (size_t)t + k])) flag = 1;
        }
        const float rec[12] = {T[0], T[1], T[2], asf(flag), T[3], T[4], T[5], 0.0f, T[6], T[7], T[8], 0.0f};
        std::copy(rec, rec + 12, &outTri[12 * (size_t)t]);
    }
    for (int i = 0; i < nEl; i++) {
        const float* E = &el[10 * (size_t)i];
        int flag = 0;
        if (then) {
            flag = i < then->nEl ? 0 : 1;
            for (int k = 0; k < 10 && !flag; k++) if (!(E[k] == then->el[10 * (size_t)i + k])) flag = 1;
            if (flag && i < then->nEl)
                for (int k = 6; k < 9; k++) if (E[k] != 0.0f || then->el[10 * (size_t)i + k] != 0.0f) flag = 2;
        }
        const float rec[12] = {E[0], E[1], E[2], E[9], E[3], E[4], E[5], asf(flag), E[6], E[7], E[8], 0.0f};
        std::copy(rec, rec + 12, &outEl[12 * (size_t)i]);
    }
}

}  // namespace ptp
