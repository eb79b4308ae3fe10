// pt_rig_mix_rule.hpp — the host-only part of include/pt_rig_mix.h: what its calls refuse in their arguments before their first HIP call (the
// first failing check as a code and one text each, in the header's order), the loop wrap of a layer's time, the (ka, kb, u) a layer hands the
// kernel, and ptp::rigMix, a plain C++ statement of steps 2-7 that k_rig_mix (pt_rig_mix.hip) is the device statement of.  The key blend and
// the interval are pt_rig_rule.hpp's (ptp::rigBlend, ptp::rigInterval), used and not restated.  Plain C++: no HIP runtime call and no context, so
// tests/c/rig_mix_rule_check.cpp runs all of it on a CPU.  Whether a rig is live, whose its pose is and which slots are filled are the
// registry's and the rig's to say (pt_rig_host.hpp); they arrive here as answers.  Binary32 throughout, every product rounded before every
// sum, in the written order (the file is compiled with -ffp-contract=off wherever it is compiled).
#pragma once
#include "../../../include/pt_rig_mix.h"
#include "pt_rig_rule.hpp"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

namespace ptp {

// every check below, in the order the header lists them (the test requires each of them of its grid)
enum RigMixCheck { RX_OK, RX_NULL, RX_RIG, RX_FOREIGN, RX_SLOT, RX_N_KEYS, RX_CLIP_NULL, RX_TIME_BYTES, RX_VALUE_BYTES, RX_TIMES, RX_MASK_SLOT, RX_WEIGHTS, RX_WEIGHT_BYTES,
                   RX_WEIGHT, RX_LAYERS, RX_LAYER_BYTES, RX_L_CLIP, RX_L_MASK, RX_L_MODE, RX_L_WRAP, RX_L_NAN_T, RX_L_INF_T, RX_L_WEIGHT, RX_BASE, RX_OUT, RX_OUT_BYTES,
                   RX_ELLIP_BYTES, RX_COUNT };

// which slots of a rig are filled: the keys of each clip slot (0: empty) and whether each mask slot is set
struct RigMixSlots {
    int nKeys[PT_RIG_MIX_SLOTS] = {};
    bool mask[PT_RIG_MIX_MASKS] = {};
};

namespace rig_mix_detail {
inline Refused refuse(const char* who, int* which, RigMixCheck k, const std::string& text) {
    if (which) *which = k;
    return Refused{PT_ERR_ARG, std::string(who) + ": " + text};
}
inline bool unitWeight(float w) { return std::isfinite(w) && w >= 0.0f && w <= 1.0f; }
}  // namespace rig_mix_detail

// pt_rig_mix_clip; live: the rig is neither null nor destroyed; nParts: its pose's (read only when live).  After the slot, pt_rig_clip_attach's
// checks under this name
inline Refused checkRigMixClip(bool live, int slot, int nKeys, const float* times, size_t timeBytes, const float* values, size_t valueBytes, int nParts, int* which = nullptr) {
    using rig_mix_detail::refuse;
    const char* who = "pt_rig_mix_clip";
    if (which) *which = RX_OK;
    if (!live) return refuse(who, which, RX_RIG, "null or destroyed rig");
    if (slot < 0 || slot >= PT_RIG_MIX_SLOTS) return refuse(who, which, RX_SLOT, "a slot outside [0, 16)");
    if (nKeys < 1) return refuse(who, which, RX_N_KEYS, "n_keys < 1");
    if (!times || (!values && nParts > 0)) return refuse(who, which, RX_CLIP_NULL, "null times, or null values with n_parts > 0");
    if (timeBytes != (size_t)nKeys * 4) return refuse(who, which, RX_TIME_BYTES, "time_bytes != n_keys * 4");
    if (valueBytes != (size_t)nKeys * (size_t)nParts * (PT_RIG_LOCAL_FLOATS * 4)) return refuse(who, which, RX_VALUE_BYTES, "value_bytes != n_keys * n_parts * 48");
    for (int k = 0; k < nKeys; k++)
        if (!std::isfinite(times[k]) || (k > 0 && !(times[k] > times[k - 1]))) return refuse(who, which, RX_TIMES, "times must be finite and strictly increasing");
    return {};
}

// pt_rig_mix_mask
inline Refused checkRigMixMask(bool live, int slot, const float* weights, size_t weightBytes, int nParts, int* which = nullptr) {
    using rig_mix_detail::refuse;
    const char* who = "pt_rig_mix_mask";
    if (which) *which = RX_OK;
    if (!live) return refuse(who, which, RX_RIG, "null or destroyed rig");
    if (slot < 0 || slot >= PT_RIG_MIX_MASKS) return refuse(who, which, RX_MASK_SLOT, "a slot outside [0, 8)");
    if (!weights && nParts > 0) return refuse(who, which, RX_WEIGHTS, "null weights with n_parts > 0");
    if (weightBytes != (size_t)nParts * 4) return refuse(who, which, RX_WEIGHT_BYTES, "weight_bytes != n_parts * 4");
    for (int j = 0; j < nParts; j++)
        if (!rig_mix_detail::unitWeight(weights[j])) return refuse(who, which, RX_WEIGHT, "a weight must be finite and in [0, 1]");
    return {};
}

// the three layer calls
enum RigMixCall { RIG_MIX_LOCALS, RIG_MIX_RECORDS, RIG_MIX_GEOMETRY };
inline const char* rigMixName(RigMixCall call) {
    return call == RIG_MIX_LOCALS ? "pt_rig_mix_locals" : call == RIG_MIX_RECORDS ? "pt_rig_mix_records" : "pt_rig_mix_pose_geometry";
}

// ctx and own are read for the geometry call only; slots and nParts only when live; out / outBytes are locals_out or records_out and their byte
// count, for the geometry call ellip and ellip_bytes
inline Refused checkRigMixLayers(RigMixCall call, const void* ctx, bool live, bool own, const RigMixSlots& slots, const pt_rig_layer* layers, size_t layerBytes,
                                 const float* out, size_t outBytes, int nParts, int* which = nullptr) {
    using rig_mix_detail::refuse;
    const char* who = rigMixName(call);
    if (which) *which = RX_OK;
    if (call == RIG_MIX_GEOMETRY && !ctx) return refuse(who, which, RX_NULL, "null ctx");
    if (!live) return refuse(who, which, RX_RIG, "null or destroyed rig");
    if (call == RIG_MIX_GEOMETRY && !own) return refuse(who, which, RX_FOREIGN, "the rig's pose was created on another context");
    if (!layers) return refuse(who, which, RX_LAYERS, "null layers");
    if (layerBytes % sizeof(pt_rig_layer) || layerBytes < sizeof(pt_rig_layer) || layerBytes > PT_RIG_MIX_MAX_LAYERS * sizeof(pt_rig_layer))
        return refuse(who, which, RX_LAYER_BYTES, "layer_bytes must be 24 times a layer count of 1 to 8");
    const int n = (int)(layerBytes / sizeof(pt_rig_layer));
    for (int l = 0; l < n; l++) {
        const pt_rig_layer& y = layers[l];
        const std::string at = "layer " + std::to_string(l) + ": ";
        if (y.clip < 0 || y.clip >= PT_RIG_MIX_SLOTS || slots.nKeys[y.clip] < 1) return refuse(who, which, RX_L_CLIP, at + "a clip slot outside [0, 16) or empty");
        if (y.mask < -1 || y.mask >= PT_RIG_MIX_MASKS || (y.mask >= 0 && !slots.mask[y.mask])) return refuse(who, which, RX_L_MASK, at + "a mask outside [-1, 8) or empty");
        if (y.mode != PT_RIG_MIX_OVERRIDE && y.mode != PT_RIG_MIX_ADDITIVE) return refuse(who, which, RX_L_MODE, at + "unknown mode");
        if (y.wrap != PT_RIG_MIX_CLAMP && y.wrap != PT_RIG_MIX_LOOP) return refuse(who, which, RX_L_WRAP, at + "unknown wrap");
        if (y.t != y.t) return refuse(who, which, RX_L_NAN_T, at + "t is NaN");
        if (y.wrap == PT_RIG_MIX_LOOP && std::isinf(y.t)) return refuse(who, which, RX_L_INF_T, at + "an infinite t with LOOP");
        if (!rig_mix_detail::unitWeight(y.weight)) return refuse(who, which, RX_L_WEIGHT, at + "a weight must be finite and in [0, 1]");
    }
    if (layers[0].mode != PT_RIG_MIX_OVERRIDE || layers[0].mask != -1 || layers[0].weight != 1.0f)
        return refuse(who, which, RX_BASE, "layer 0 must be OVERRIDE with mask -1 and weight 1");
    if (call == RIG_MIX_GEOMETRY) {
        if (out && outBytes % 4) return refuse(who, which, RX_ELLIP_BYTES, "ellip_bytes must be a multiple of 4 bytes");
        return {};
    }
    const bool locals = call == RIG_MIX_LOCALS;
    if (!out) return refuse(who, which, RX_OUT, locals ? "null locals_out" : "null records_out");
    if (outBytes != (size_t)nParts * (locals ? PT_RIG_LOCAL_FLOATS * 4 : PT_POSE_RECORD_FLOATS * 4))
        return refuse(who, which, RX_OUT_BYTES, locals ? "local_bytes != n_parts * 48" : "record_bytes != n_parts * 96");
    return {};
}

// STEP 1, the loop wrap: the time of a LOOP layer in a clip of nKeys > 1 strictly increasing finite times; t is finite
inline float rigMixWrap(const float* times, int nKeys, float t) {
    const float D = times[nKeys - 1] - times[0];
    const float x = t - times[0];
    float r = std::fmod(x, D);
    if (r < 0.0f) r = r + D;
    return times[0] + r;
}

// STEP 1: what a layer hands the kernel.  At a key, or clamped, ka == kb is that key and u == 0
struct RigMixStep { int ka = 0, kb = 0; float u = 0.0f; };
inline RigMixStep rigMixStep(const float* times, int nKeys, int wrap, float t) {
    RigMixStep s;
    if (nKeys == 1) return s;
    if (wrap == PT_RIG_MIX_LOOP) t = rigMixWrap(times, nKeys, t);
    int k; float u;
    const int exact = rigInterval(times, nKeys, t, &k, &u);
    if (exact >= 0) { s.ka = s.kb = exact; return s; }
    s.ka = k; s.kb = k + 1; s.u = u;
    return s;
}

// a layer as steps 2-7 read it: the locals of keys ka, kb and 0 of its slot (n joints each), its mask (n floats) or null, u, weight and mode
struct RigMixLayer { const float* a = nullptr; const float* b = nullptr; const float* r = nullptr; const float* mask = nullptr; float u = 0.0f, weight = 1.0f; int mode = 0; };

// p (x) q on (x y z w), in the header's order
inline void rigQuatMul(const float* p, const float* q, float* o) {
    const float px = p[0], py = p[1], pz = p[2], pw = p[3], qx = q[0], qy = q[1], qz = q[2], qw = q[3];
    const float w0 = pw * qw, w1 = px * qx, w2 = py * qy, w3 = pz * qz;
    const float x0 = pw * qx, x1 = px * qw, x2 = py * qz, x3 = pz * qy;
    const float y0 = pw * qy, y1 = px * qz, y2 = py * qw, y3 = pz * qx;
    const float z0 = pw * qz, z1 = px * qy, z2 = py * qx, z3 = pz * qw;
    o[0] = ((x0 + x1) + x2) - x3;
    o[1] = ((y0 - y1) + y2) + y3;
    o[2] = ((z0 + z1) - z2) + z3;
    o[3] = ((w0 - w1) - w2) - w3;
}

// STEPS 2-7: the mixed locals of n joints under nLayers >= 1 checked layers, 12 floats per joint into out
inline void rigMix(const RigMixLayer* layers, int nLayers, size_t n, float* out) {
    constexpr int F = PT_RIG_LOCAL_FLOATS;
    for (size_t j = 0; j < n; j++) {
        float acc[F], S[F], tmp[F];
        for (int l = 0; l < nLayers; l++) {
            const RigMixLayer& y = layers[l];
            if (y.u == 0.0f) { for (int f = 0; f < F; f++) S[f] = y.a[F * j + f]; }      // step 2: the key's own, bit for bit
            else rigBlend(y.a + F * j, y.b + F * j, y.u, 1, S);
            if (l == 0) { for (int f = 0; f < F; f++) acc[f] = S[f]; continue; }         // step 4
            const float e = y.mask ? y.weight * y.mask[j] : y.weight;                      // step 3
            if (e == 0.0f) continue;
            if (y.mode == PT_RIG_MIX_OVERRIDE) {                                           // step 5
                if (e == 1.0f) { for (int f = 0; f < F; f++) acc[f] = S[f]; continue; }
                rigBlend(acc, S, e, 1, tmp);
                for (int f = 0; f < F; f++) acc[f] = tmp[f];
                continue;
            }
            const float* R = y.r + F * j;                                                  // step 6
            for (int f = 0; f < F; f++) {
                if (f >= 4 && f < 8) continue;
                const float d = S[f] - R[f];
                const float p = e * d;
                acc[f] = acc[f] + p;
            }
            const float conj[4] = {-R[4], -R[5], -R[6], R[7]};
            float dq[4];
            rigQuatMul(S + 4, conj, dq);
            if (dq[3] < 0.0f) { for (int f = 0; f < 4; f++) dq[f] = -dq[f]; }
            const float v = 1.0f - e, ew = e * dq[3];
            const float dp[4] = {e * dq[0], e * dq[1], e * dq[2], v + ew};
            rigQuatMul(dp, acc + 4, tmp);
            for (int f = 0; f < 4; f++) acc[4 + f] = tmp[f];
        }
        for (int f = 0; f < F; f++) out[F * j + f] = acc[f];
        out[F * j + 3] = out[F * j + 11] = 0.0f;                                           // step 7
    }
}

}  // namespace ptp
