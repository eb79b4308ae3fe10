// pt_skin_dq_rule.hpp — the host-only part of include/pt_skin_dq.h: a plain C++ statement of the rule that k_dq_records and k_skin_dq_corners
// (pt_skin_dq.hip) are the device statements of.  The argument checks are pt_skin_rule.hpp's (ptp::checkSkinCreate under the name
// pt_skin_dq_create); the last step is ptp::poseQuad as it stands, on the record the blended dual quaternion turns back into.  Plain C++: no HIP
// runtime call and no context, so tests/c/skin_dq_rule_check.cpp runs all of it on a CPU.  Binary32 throughout, every product rounded before every
// sum, in the written order (the file is compiled with -ffp-contract=off wherever it is compiled); sqrt and / are correctly rounded.
#pragma once
#include "../../../include/pt_skin_dq.h"
#include "pt_skin_rule.hpp"

#include <cmath>
#include <vector>

namespace ptp {

constexpr int DQ_FLOATS = 8;            // a record as a dual quaternion: (w x y z)(dw dx dy dz)

// STEP 1: floats 0-11 of a record -> its dual quaternion.  Which of the four branches ran is returned (0: the trace, 1-3: the largest diagonal)
inline int dqFromRecord(const float* X, float* q) {
    const float m00 = X[0], m01 = X[1], m02 = X[2], tx = X[3], m10 = X[4], m11 = X[5], m12 = X[6], ty = X[7], m20 = X[8], m21 = X[9], m22 = X[10], tz = X[11];
    const float tr = (m00 + m11) + m22;
    float w, x, y, z;
    int branch;
    if (tr > 0.0f) {
        const float s = std::sqrt(tr + 1.0f) * 2.0f;
        w = 0.25f * s; x = (m21 - m12) / s; y = (m02 - m20) / s; z = (m10 - m01) / s;
        branch = 0;
    } else if (m00 > m11 && m00 > m22) {
        const float s = std::sqrt(((1.0f + m00) - m11) - m22) * 2.0f;
        w = (m21 - m12) / s; x = 0.25f * s; y = (m01 + m10) / s; z = (m02 + m20) / s;
        branch = 1;
    } else if (m11 > m22) {
        const float s = std::sqrt(((1.0f + m11) - m00) - m22) * 2.0f;
        w = (m02 - m20) / s; x = (m01 + m10) / s; y = 0.25f * s; z = (m12 + m21) / s;
        branch = 2;
    } else {
        const float s = std::sqrt(((1.0f + m22) - m00) - m11) * 2.0f;
        w = (m10 - m01) / s; x = (m02 + m20) / s; y = (m12 + m21) / s; z = 0.25f * s;
        branch = 3;
    }
    const float ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    const float n = std::sqrt(((ww + xx) + yy) + zz);
    w = w / n; x = x / n; y = y / n; z = z / n;
    q[0] = w; q[1] = x; q[2] = y; q[3] = z;
    float a = tx * x, b = ty * y, c = tz * z;
    q[4] = -0.5f * ((a + b) + c);
    a = tx * w; b = ty * z; c = tz * y;
    q[5] = 0.5f * ((a + b) - c);
    a = ty * w; b = tz * x; c = tx * z;
    q[6] = 0.5f * ((a + b) - c);
    a = tz * w; b = tx * y; c = ty * x;
    q[7] = 0.5f * ((a + b) - c);
    return branch;
}

// STEP 2: the blend of one corner from its four slots over the table of dual quaternions (8 floats per bone), normalised: r and d, 4 floats
// each.  At least slot 0 is used; the weights of empty slots are never multiplied.  Returns the slots whose weight was negated, as bits.
inline int dqBlend(const int32_t* b, const float* w, const float* table, float* r, float* d) {
    const float* Q0 = table + (size_t)DQ_FLOATS * (size_t)b[0];
    float Br[4], Bd[4];
    for (int j = 0; j < 4; j++) { Br[j] = w[0] * Q0[j]; Bd[j] = w[0] * Q0[4 + j]; }
    int flips = 0;
    for (int s = 1; s < PT_SKIN_SLOTS && b[s] >= 0; s++) {
        const float* Q = table + (size_t)DQ_FLOATS * (size_t)b[s];
        const float p0 = Q0[0] * Q[0], p1 = Q0[1] * Q[1], p2 = Q0[2] * Q[2], p3 = Q0[3] * Q[3];
        const float dot = ((p0 + p1) + p2) + p3;
        float ws = w[s];
        if (dot < 0.0f) { ws = -ws; flips |= 1 << s; }
        for (int j = 0; j < 4; j++) {
            const float pr = ws * Q[j], pd = ws * Q[4 + j];
            Br[j] = Br[j] + pr;
            Bd[j] = Bd[j] + pd;
        }
    }
    const float ww = Br[0] * Br[0], xx = Br[1] * Br[1], yy = Br[2] * Br[2], zz = Br[3] * Br[3];
    const float L = std::sqrt(((ww + xx) + yy) + zz);
    for (int j = 0; j < 4; j++) { r[j] = Br[j] / L; d[j] = Bd[j] / L; }
    return flips;
}

// STEP 3: the unit dual quaternion back to a record B of 24 floats: M = [R | t], N = R, padding 0
inline void dqRecord(const float* r, const float* d, float* B) {
    const float w = r[0], x = r[1], y = r[2], z = r[3];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    const float R[9] = {1.0f - 2.0f * (yy + zz), 2.0f * (xy - wz), 2.0f * (xz + wy),
                        2.0f * (xy + wz), 1.0f - 2.0f * (xx + zz), 2.0f * (yz - wx),
                        2.0f * (xz - wy), 2.0f * (yz + wx), 1.0f - 2.0f * (xx + yy)};
    float t[3];
    {
        const float a = d[1] * w, b = d[0] * x, c = d[3] * y, e = d[2] * z;
        t[0] = 2.0f * (((a - b) + c) - e);
    }
    {
        const float a = d[2] * w, b = d[0] * y, c = d[1] * z, e = d[3] * x;
        t[1] = 2.0f * (((a - b) + c) - e);
    }
    {
        const float a = d[3] * w, b = d[0] * z, c = d[2] * x, e = d[1] * y;
        t[2] = 2.0f * (((a - b) + c) - e);
    }
    for (int i = 0; i < 3; i++) {
        B[4 * i] = R[3 * i]; B[4 * i + 1] = R[3 * i + 1]; B[4 * i + 2] = R[3 * i + 2]; B[4 * i + 3] = t[i];
    }
    for (int j = 0; j < 9; j++) B[12 + j] = R[j];
    B[21] = B[22] = B[23] = 0.0f;
}

// out (40 floats per triangle) = the rule applied to rest under the two tables and the pose's records (nParts of them); the tables were checked by
// checkSkinCreate.  branches (4 counters) and flips (1 counter), where given, count what the conversions and the blends took
inline void skinDqTriangles(const float* rest, const int32_t* bone, const float* weight, size_t nTris, const float* xforms, size_t nParts, float* out,
                            size_t* branches = nullptr, size_t* flips = nullptr) {
    std::vector<float> table(DQ_FLOATS * nParts + 1);
    for (size_t p = 0; p < nParts; p++) {
        const int br = dqFromRecord(xforms + (size_t)PT_POSE_RECORD_FLOATS * p, table.data() + DQ_FLOATS * p);
        if (branches) branches[br]++;
    }
    float r[4], d[4], B[PT_POSE_RECORD_FLOATS];
    for (size_t k = 0; k < nTris; k++) {
        const float* T = rest + 40 * k; float* O = out + 40 * k;
        for (int f = 0; f < 40; f++) O[f] = T[f];
        for (int c = 0; c < 3; c++) {
            const int32_t* b = bone + 12 * k + 4 * c;
            if (b[0] < 0) continue;
            const int fl = dqBlend(b, weight + 12 * k + 4 * c, table.data(), r, d);
            if (flips && fl) flips[0]++;
            dqRecord(r, d, B);
            poseQuad(B, c, T + 4 * c, O + 4 * c);
            poseQuad(B, 3 + c, T + 12 + 4 * c, O + 12 + 4 * c);
        }
    }
}

}  // namespace ptp
