// pt_rig_rule.hpp — the host-only part of include/pt_rig.h: what its calls refuse in their arguments before their first HIP call (the first
// failing check as a code and one text each, in the header's order), the depth and level plan of a hierarchy, a clip's interval and u, and a plain
// C++ statement of steps 1-5 that k_rig_level and k_rig_blend (pt_rig.hip) are the device statements of.  Plain C++: no HIP runtime call and no
// context, so tests/c/rig_rule_check.cpp runs all of it on a CPU.  Whether a rig is live and whose its pose is are the registry's to say
// (pt_rig_host.hpp); they arrive here as answers.  Binary32 throughout, every product rounded before every sum, in the written order (the file
// is compiled with -ffp-contract=off wherever it is compiled); sqrt and / are correctly rounded.
#pragma once
#include "../../../include/pt_rig.h"
#include "pt_image_history.hpp"      // ptp::Refused

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace ptp {

// every check below, in the order the header lists them (the test requires each of them of its grid)
enum RigCheck { RG_OK, RG_NULL, RG_POSE, RG_PARENT_BYTES, RG_PARENT, RG_BIND_BYTES, RG_DEPTH, RG_RIG, RG_FOREIGN, RG_LOCALS, RG_LOCAL_BYTES, RG_OUT, RG_RECORD_BYTES,
                RG_NO_CLIP, RG_NAN_T, RG_N_KEYS, RG_CLIP_NULL, RG_TIME_BYTES, RG_VALUE_BYTES, RG_TIMES, RG_ELLIP_BYTES, RG_COUNT };

namespace rig_detail {
inline Refused refuse(const char* who, int* which, RigCheck k, const char* text) {
    if (which) *which = k;
    return Refused{PT_ERR_ARG, std::string(who) + ": " + text};
}
}  // namespace rig_detail

// the depth of every joint (a root: 1) into depth, n entries; returns the rig's depth (no joints: 0).  The parents were checked to lie in [-1, j)
inline int rigDepths(const int32_t* parent, size_t n, int32_t* depth) {
    int deepest = 0;
    for (size_t j = 0; j < n; j++) {
        depth[j] = parent[j] < 0 ? 1 : depth[parent[j]] + 1;
        if (depth[j] > deepest) deepest = depth[j];
    }
    return deepest;
}

// pt_rig_create; live: the pose is live; nParts: the pose's (read only when live)
inline Refused checkRigCreate(const void* pose, bool live, const int32_t* parent, size_t parentBytes, const float* invBind, size_t bindBytes, const void* out, int nParts,
                              int* which = nullptr) {
    using rig_detail::refuse;
    const char* who = "pt_rig_create";
    if (which) *which = RG_OK;
    if (!pose || !parent || !out) return refuse(who, which, RG_NULL, "null pose, parent or out");
    if (!live) return refuse(who, which, RG_POSE, "the pose is not live");
    if (parentBytes != (size_t)nParts * 4) return refuse(who, which, RG_PARENT_BYTES, "parent_bytes != n_parts * 4");
    for (int j = 0; j < nParts; j++)
        if (parent[j] < -1 || parent[j] >= j) return refuse(who, which, RG_PARENT, "a parent outside [-1, j)");
    if (invBind && bindBytes != (size_t)nParts * (PT_RIG_LOCAL_FLOATS * 4)) return refuse(who, which, RG_BIND_BYTES, "bind_bytes != n_parts * 48");
    std::vector<int32_t> depth((size_t)nParts);
    if (rigDepths(parent, (size_t)nParts, depth.data()) > PT_RIG_MAX_DEPTH) return refuse(who, which, RG_DEPTH, "a depth above PT_RIG_MAX_DEPTH (256)");
    return {};
}

// the locals of a call, for both calls that take them
inline Refused checkRigLocals(const char* who, const float* locals, size_t localBytes, int nParts, int* which) {
    using rig_detail::refuse;
    if (!locals && nParts > 0) return refuse(who, which, RG_LOCALS, "null locals with n_parts > 0");
    if (localBytes != (size_t)nParts * (PT_RIG_LOCAL_FLOATS * 4)) return refuse(who, which, RG_LOCAL_BYTES, "local_bytes != n_parts * 48");
    return {};
}
// the time of a clip call, for both calls that take one
inline Refused checkRigTime(const char* who, bool hasClip, float t, int* which) {
    using rig_detail::refuse;
    if (!hasClip) return refuse(who, which, RG_NO_CLIP, "no clip attached");
    if (t != t) return refuse(who, which, RG_NAN_T, "t is NaN");
    return {};
}
inline Refused checkRigOut(const char* who, const float* out, size_t recordBytes, int nParts, int* which) {
    using rig_detail::refuse;
    if (!out) return refuse(who, which, RG_OUT, "null records_out");
    if (recordBytes != (size_t)nParts * (PT_POSE_RECORD_FLOATS * 4)) return refuse(who, which, RG_RECORD_BYTES, "record_bytes != n_parts * 96");
    return {};
}

// pt_rig_records; live: the rig is neither null nor destroyed; nParts: its pose's (read only when live)
inline Refused checkRigRecords(bool live, const float* locals, size_t localBytes, const float* out, size_t recordBytes, int nParts, int* which = nullptr) {
    const char* who = "pt_rig_records";
    if (which) *which = RG_OK;
    if (!live) return rig_detail::refuse(who, which, RG_RIG, "null or destroyed rig");
    if (Refused r = checkRigLocals(who, locals, localBytes, nParts, which); r.code) return r;
    return checkRigOut(who, out, recordBytes, nParts, which);
}

// pt_rig_clip_records
inline Refused checkRigClipRecords(bool live, bool hasClip, float t, const float* out, size_t recordBytes, int nParts, int* which = nullptr) {
    const char* who = "pt_rig_clip_records";
    if (which) *which = RG_OK;
    if (!live) return rig_detail::refuse(who, which, RG_RIG, "null or destroyed rig");
    if (Refused r = checkRigTime(who, hasClip, t, which); r.code) return r;
    return checkRigOut(who, out, recordBytes, nParts, which);
}

// pt_rig_clip_attach
inline Refused checkRigClipAttach(bool live, int nKeys, const float* times, size_t timeBytes, const float* values, size_t valueBytes, int nParts, int* which = nullptr) {
    using rig_detail::refuse;
    const char* who = "pt_rig_clip_attach";
    if (which) *which = RG_OK;
    if (!live) return refuse(who, which, RG_RIG, "null or destroyed rig");
    if (nKeys < 1) return refuse(who, which, RG_N_KEYS, "n_keys < 1");
    if (!times || (!values && nParts > 0)) return refuse(who, which, RG_CLIP_NULL, "null times, or null values with n_parts > 0");
    if (timeBytes != (size_t)nKeys * 4) return refuse(who, which, RG_TIME_BYTES, "time_bytes != n_keys * 4");
    if (valueBytes != (size_t)nKeys * (size_t)nParts * (PT_RIG_LOCAL_FLOATS * 4)) return refuse(who, which, RG_VALUE_BYTES, "value_bytes != n_keys * n_parts * 48");
    for (int k = 0; k < nKeys; k++)
        if (!std::isfinite(times[k]) || (k > 0 && !(times[k] > times[k - 1]))) return refuse(who, which, RG_TIMES, "times must be finite and strictly increasing");
    return {};
}

// pt_rig_pose_geometry (clip false) and pt_rig_clip_pose_geometry (clip true: locals and localBytes are not read); own: the rig's pose was created on ctx
inline Refused checkRigGeometry(bool clip, const void* ctx, bool live, bool own, const float* locals, size_t localBytes, bool hasClip, float t, int nParts, const float* ellip,
                                size_t ellipBytes, int* which = nullptr) {
    using rig_detail::refuse;
    const char* who = clip ? "pt_rig_clip_pose_geometry" : "pt_rig_pose_geometry";
    if (which) *which = RG_OK;
    if (!ctx) return refuse(who, which, RG_NULL, "null ctx");
    if (!live) return refuse(who, which, RG_RIG, "null or destroyed rig");
    if (!own) return refuse(who, which, RG_FOREIGN, "the rig's pose was created on another context");
    if (Refused r = clip ? checkRigTime(who, hasClip, t, which) : checkRigLocals(who, locals, localBytes, nParts, which); r.code) return r;
    if (ellip && ellipBytes % 4) return refuse(who, which, RG_ELLIP_BYTES, "ellip_bytes must be a multiple of 4 bytes");
    return {};
}

// THE LEVEL PLAN: the joints sorted by (depth, id), and where each level starts in that order (levels + 1 entries; no joints: one entry, 0).
// Level l holds the joints of depth l + 1: a level's parents all lie in the level before it.
struct RigPlan {
    std::vector<int32_t> order, levelStart;
    int levels() const { return (int)levelStart.size() - 1; }
};
inline void rigPlan(const int32_t* parent, size_t n, RigPlan& plan) {
    std::vector<int32_t> depth(n);
    const int levels = rigDepths(parent, n, depth.data());
    plan.levelStart.assign((size_t)levels + 1, 0);
    for (size_t j = 0; j < n; j++) plan.levelStart[(size_t)depth[j]]++;          // counts, shifted by one
    for (int l = 0; l < levels; l++) plan.levelStart[(size_t)l + 1] += plan.levelStart[(size_t)l];
    plan.order.resize(n);
    std::vector<int32_t> at(plan.levelStart.begin(), plan.levelStart.end() - (levels ? 1 : 0));
    for (size_t j = 0; j < n; j++) plan.order[(size_t)at[(size_t)depth[j] - 1]++] = (int32_t)j;      // ascending j within a level
}

// STEP 5, the host's part: the interval k and u of a time in a clip of nKeys >= 1 strictly increasing finite times; t is no NaN.  Returns which key
// the locals are (*exact >= 0: no blend, that key bit for bit) or -1 (*k and *u say what to blend)
inline int rigInterval(const float* times, int nKeys, float t, int* k, float* u) {
    *k = 0; *u = 0.0f;
    if (nKeys == 1) return 0;
    if (t < times[0]) t = times[0];
    if (t > times[nKeys - 1]) t = times[nKeys - 1];
    int lo = 0;
    while (lo < nKeys - 2 && !(t < times[lo + 1])) lo++;              // T_lo <= t < T_lo+1, or the last interval
    const float num = t - times[lo], den = times[lo + 1] - times[lo];
    *k = lo; *u = num / den;
    if (*u == 0.0f) return lo;
    if (*u == 1.0f) return lo + 1;
    return -1;
}

// STEP 5, the blend of n joints' locals: out = a and b under u (neither 0 nor 1).  The padding floats come out as the blend of the paddings
inline void rigBlend(const float* a, const float* b, float u, size_t n, float* out) {
    const float v = 1.0f - u;
    for (size_t j = 0; j < n; j++) {
        const float* A = a + PT_RIG_LOCAL_FLOATS * j; const float* B = b + PT_RIG_LOCAL_FLOATS * j; float* O = out + PT_RIG_LOCAL_FLOATS * j;
        const float p0 = A[4] * B[4], p1 = A[5] * B[5], p2 = A[6] * B[6], p3 = A[7] * B[7];
        const float d = ((p0 + p1) + p2) + p3;
        const float uq = d < 0.0f ? -u : u;
        for (int f = 0; f < PT_RIG_LOCAL_FLOATS; f++) {
            const float w = f >= 4 && f < 8 ? uq : u;
            const float x = v * A[f], y = w * B[f];
            O[f] = x + y;
        }
    }
}

// STEP 1: a local -> L, 12 floats, rows (l_i0 l_i1 l_i2 t_i)
inline void rigLocal(const float* l, float* L) {
    float x = l[4], y = l[5], z = l[6], w = l[7];
    const float xx0 = x * x, yy0 = y * y, zz0 = z * z, ww0 = w * w;
    const float n = std::sqrt(((xx0 + yy0) + zz0) + ww0);
    x = x / n; y = y / n; z = z / n; w = w / n;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    const float R[9] = {1.0f - 2.0f * (yy + zz), 2.0f * (xy - wz), 2.0f * (xz + wy),
                        2.0f * (xy + wz), 1.0f - 2.0f * (xx + zz), 2.0f * (yz - wx),
                        2.0f * (xz - wy), 2.0f * (yz + wx), 1.0f - 2.0f * (xx + yy)};
    for (int i = 0; i < 3; i++) {
        for (int c = 0; c < 3; c++) L[4 * i + c] = R[3 * i + c] * l[8 + c];
        L[4 * i + 3] = l[i];
    }
}

// STEPS 2 and 3: C = A o B on 3 x 4 matrices (C is neither A nor B)
inline void rigCompose(const float* A, const float* B, float* C) {
    for (int i = 0; i < 3; i++) {
        const float a0 = A[4 * i], a1 = A[4 * i + 1], a2 = A[4 * i + 2], a3 = A[4 * i + 3];
        for (int k = 0; k < 4; k++) {
            const float p0 = a0 * B[k], p1 = a1 * B[4 + k], p2 = a2 * B[8 + k];
            const float s = (p0 + p1) + p2;
            C[4 * i + k] = k < 3 ? s : s + a3;
        }
    }
}

// STEP 4: the record of M (12 floats): M, then N, then three zeros
inline void rigRecord(const float* M, float* rec) {
    for (int f = 0; f < 12; f++) rec[f] = M[f];
    float c[9];
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, k1 = (k + 1) % 3, k2 = (k + 2) % 3;
            const float p = M[4 * i1 + k1] * M[4 * i2 + k2], q = M[4 * i1 + k2] * M[4 * i2 + k1];
            c[3 * i + k] = p - q;
        }
    const float d0 = M[0] * c[0], d1 = M[1] * c[1], d2 = M[2] * c[2];
    const float det = (d0 + d1) + d2;
    for (int f = 0; f < 9; f++) rec[12 + f] = c[f] / det;
    rec[21] = rec[22] = rec[23] = 0.0f;
}

// STEPS 1-4 over a hierarchy of n joints: world (12 floats per joint) and records (24 per joint) from the locals; invBind may be null
inline void rigRecords(const int32_t* parent, size_t n, const float* invBind, const float* locals, float* world, float* records) {
    float L[12], M[12];
    for (size_t j = 0; j < n; j++) {                                 // (parents come first: the order of the ids is a valid order of the levels)
        float* W = world + 12 * j;
        rigLocal(locals + PT_RIG_LOCAL_FLOATS * j, L);
        if (parent[j] < 0) { for (int f = 0; f < 12; f++) W[f] = L[f]; }
        else rigCompose(world + 12 * (size_t)parent[j], L, W);
        if (invBind) { rigCompose(W, invBind + 12 * j, M); rigRecord(M, records + PT_POSE_RECORD_FLOATS * j); }
        else rigRecord(W, records + PT_POSE_RECORD_FLOATS * j);
    }
}

// STEP 5 then 1-4: the records of a clip (nKeys * n locals, key-major) at time t
inline void rigClipRecords(const int32_t* parent, size_t n, const float* invBind, const float* times, int nKeys, const float* values, float t, float* world,
                           float* records) {
    int k; float u;
    const int exact = rigInterval(times, nKeys, t, &k, &u);
    if (exact >= 0) { rigRecords(parent, n, invBind, values + PT_RIG_LOCAL_FLOATS * n * (size_t)exact, world, records); return; }
    std::vector<float> blended(PT_RIG_LOCAL_FLOATS * n + 1);
    rigBlend(values + PT_RIG_LOCAL_FLOATS * n * (size_t)k, values + PT_RIG_LOCAL_FLOATS * n * (size_t)(k + 1), u, n, blended.data());
    rigRecords(parent, n, invBind, blended.data(), world, records);
}

}  // namespace ptp
