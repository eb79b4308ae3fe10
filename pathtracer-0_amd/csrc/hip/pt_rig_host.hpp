// pt_rig_host.hpp — the rig object behind the C ABI: the entry points of include/pt_rig.h, include/pt_rig_mix.h and include/pt_rig_ik.h (their
// timers are pt_geom_debug_host.hpp's).  Included at the end of pt_image.hpp after pt_pose_host.hpp, inside pt_hip.hip's extern "C" block; not a translation unit.
//
// It takes: the kernels behind pt_rig_launch.hpp (the key blend, one launch per level of the hierarchy) and pt_rig_mix_launch.hpp (the mix's one
// launch) and pt_rig_ik_launch.hpp (the solve's one launch); the argument checks, level plan, clip interval, loop wrap, independence check and
// level window of pt_rig_rule.hpp, pt_rig_mix_rule.hpp and pt_rig_ik_rule.hpp; and from
// pt_pose_host.hpp poseGeometry, poseLive, the registry mutex, staleRefused and the pose's plan, on whose stream a rig does all its work.
//
// What a reader must know.  A rig belongs to a pose of any rule and makes that pose's records on the device.  Every record call reads: check,
// source, tail.  A source (localsFromCaller, localsFromClip, localsFromMix) makes the call's locals available on the device and returns where;
// all three share dLocals, except that a time at a key reads that key's locals in the clip, in place.  A tail runs the levels over them into dR
// and downloads the records (rigRecords), or does that and hands them to poseGeometry with dR as the records on the device (rigGeometry).
// While goals are set (pt_rig_ik_goals) over a table with constraints, one stage sits between source and levels: rigLevels runs it.  It brings
// the locals into dLocals if the source answered elsewhere (a clip's keys are never written), runs the levels that make the first joints'
// parents' world matrices, then k_rig_ik on dLocals, then the levels from the shallowest first joint down (ptp::RigIkWindow).
// A rig without joints enqueues nothing.  Every call ends with the plan's stream idle.
extern "C++" {
#include "pt_rig_ik_launch.hpp"
#include "pt_rig_ik_rule.hpp"
#include "pt_rig_launch.hpp"
#include "pt_rig_mix_launch.hpp"
#include "pt_rig_mix_rule.hpp"
#include "pt_rig_rule.hpp"
}
#include "../../../include/pt_rig.h"
#include "../../../include/pt_rig_ik.h"
#include "../../../include/pt_rig_mix.h"

// a rig of include/pt_rig.h: one joint per record of its pose
struct pt_rig {
    // a keyed clip as a rig keeps it: its own (include/pt_rig.h step 5) and each slot's (include/pt_rig_mix.h)
    struct Clip {
        std::vector<float> times;       // one per key: none until a clip is attached
        Dev<float> dKeys;               // n_keys * n locals, key-major
        int nKeys() const { return (int)times.size(); }
    };
    pt_pose* pose = nullptr;
    int n = 0;                          // joints == the pose's n_parts
    ptp::RigPlan plan;                  // the joints by (depth, id) and the level starts
    bool hasBind = false;
    Dev<int32_t> dOrder, dParent;       // the plan's order; the parents by joint id
    Dev<float> dBind, dLocals, dW, dR;  // 12 floats per joint: the inverse binds, the locals of a call (a clip's blend, a mix), the world matrices; the records, 24 per joint
    Clip clip;                          // pt_rig_clip_attach's
    Clip mixClip[PT_RIG_MIX_SLOTS];     // pt_rig_mix_clip's
    Dev<float> dMixMask[PT_RIG_MIX_MASKS];      // pt_rig_mix_mask's, n floats each
    ptp::RigMixSlots slots;             // which slots are filled, as the checks of pt_rig_mix_rule.hpp take it: kept in step with the two lines above
    std::vector<int32_t> parent;        // the parents by joint id, as dParent holds them: what pt_rig_ik_attach checks against
    size_t nIk = 0;                     // the constraints of pt_rig_ik_attach's table
    ptp::RigIkWindow ikWindow;          // the levels around the solve
    Dev<int32_t> dIkRows;               // ptp::RigIkRow, 16 bytes per constraint
    Dev<float> dIkCons, dIkGoals;       // the table and pt_rig_ik_goals', 32 bytes per constraint each
    bool ikGoals = false;               // goals are set
    bool ikActive() const { return ikGoals && nIk > 0; }
};

namespace {

constexpr size_t JOINT_BYTES = PT_RIG_LOCAL_FLOATS * 4;      // a joint's locals; its inverse bind and its world matrix are as large

std::set<pt_rig*> g_rigs;               // the live rigs, under g_posesMutex: a rig leaves with its pose at the latest
bool rigLive(pt_rig* r) {
    std::lock_guard<std::mutex> g(g_posesMutex);
    return r && g_rigs.count(r);
}

void rigsFree(pt_pose* P) {
    {
        std::lock_guard<std::mutex> g(g_posesMutex);
        for (pt_rig* r : P->rigs) g_rigs.erase(r);
    }
    for (pt_rig* r : P->rigs) delete r;
}

// THE store of a table of the rig (a clip's keys, a mask): staged, uploaded and synchronised on the plan's stream, then moved into place — the
// rig changes only once the allocation stands
extern "C++" template <class T>
int rigStore(pt_rig* G, const void* values, size_t bytes, Dev<T>& into) {
    const hipStream_t st = G->pose->plan->stream;
    HIP_TRY(hipSetDevice(G->pose->device));
    Dev<T> staged;
    HIP_TRY(staged.upload(values, bytes, st));
    HIP_TRY(hipStreamSynchronize(st));
    into = std::move(staged);
    return 0;
}

// the layers of a mix call checked under that call's name (c is read for the geometry call only): the refusal, or 0
int mixRefused(ptp::RigMixCall call, pt_ctx* c, pt_rig* G, const pt_rig_layer* layers, size_t layerBytes, const float* out, size_t outBytes) {
    const bool live = rigLive(G);
    return fail(ptp::checkRigMixLayers(call, c, live, live && G->pose->ctx == c, live ? G->slots : ptp::RigMixSlots(), layers, layerBytes, out, outBytes, live ? G->n : 0));
}

// include/pt_rig_mix.h step 1 for every layer, and where its keys lie: the table k_rig_mix takes by value.  The layers were checked
PtRigMixTable rigMixTable(pt_rig* G, const pt_rig_layer* layers, size_t layerBytes) {
    PtRigMixTable T = {};
    const size_t keyFloats = (size_t)G->n * PT_RIG_LOCAL_FLOATS;
    T.nLayers = (int32_t)(layerBytes / sizeof(pt_rig_layer));
    for (int l = 0; l < T.nLayers; l++) {
        const pt_rig_layer& y = layers[l];
        const pt_rig::Clip& clip = G->mixClip[y.clip];
        const ptp::RigMixStep s = ptp::rigMixStep(clip.times.data(), clip.nKeys(), y.wrap, y.t);
        const float* keys = clip.dKeys;
        T.a[l] = keys + keyFloats * (size_t)s.ka; T.b[l] = keys + keyFloats * (size_t)s.kb; T.r[l] = keys;
        T.mask[l] = y.mask >= 0 ? (const float*)G->dMixMask[y.mask] : nullptr;
        T.u[l] = s.u; T.weight[l] = y.weight; T.mode[l] = y.mode;
    }
    return T;
}

// ---- the sources: each selects the pose's device, makes a call's locals available there, asynchronously on the plan's stream, and returns where
// rigRun reads them (a rig without joints: nothing enqueued).  nullptr: a HIP call failed, and fail() has recorded which; the tails hand that on

// the caller's (host), uploaded
const float* localsFromCaller(pt_rig* G, const float* locals) {
    const auto enqueue = [&]() {
        HIP_TRY(hipSetDevice(G->pose->device));
        if (G->n) HIP_TRY(hipMemcpyAsync(G->dLocals, locals, (size_t)G->n * JOINT_BYTES, hipMemcpyHostToDevice, G->pose->plan->stream));
        return 0;
    };
    return enqueue() ? nullptr : (const float*)G->dLocals;
}

// the rig's own clip at time t (no NaN): at a key, or clamped, that key's own locals where they lie, bit for bit; else the blend of the two around t
const float* localsFromClip(pt_rig* G, float t) {
    const float* at = G->dLocals;
    const auto enqueue = [&]() {
        HIP_TRY(hipSetDevice(G->pose->device));
        if (G->n == 0) return 0;
        const size_t keyFloats = (size_t)G->n * PT_RIG_LOCAL_FLOATS;
        const float* keys = G->clip.dKeys;
        int k; float u;
        const int exact = ptp::rigInterval(G->clip.times.data(), G->clip.nKeys(), t, &k, &u);
        if (exact >= 0) at = keys + keyFloats * (size_t)exact;
        else HIP_TRY(ptRigBlendLaunch(keys + keyFloats * (size_t)k, keys + keyFloats * (size_t)(k + 1), u, G->n, G->dLocals, G->pose->plan->stream));
        return 0;
    };
    return enqueue() ? nullptr : at;
}

// the mix of a table's layers
const float* localsFromMix(pt_rig* G, const PtRigMixTable& mix) {
    const auto enqueue = [&]() {
        HIP_TRY(hipSetDevice(G->pose->device));
        if (G->n) HIP_TRY(ptRigMixLaunch(mix, G->n, G->dLocals, G->pose->plan->stream));
        return 0;
    };
    return enqueue() ? nullptr : (const float*)G->dLocals;
}

// ---- the tails

// steps 1-4 over the locals at `at` (device) into `records`, the levels [from, to) from the roots down; asynchronous on the plan's stream
int rigRunLevels(pt_rig* G, const float* at, float* records, int from, int to) {
    const hipStream_t st = G->pose->plan->stream;
    for (int l = from; l < to; l++) {
        const int first = G->plan.levelStart[(size_t)l], count = G->plan.levelStart[(size_t)l + 1] - first;
        HIP_TRY(ptRigLevelLaunch(G->dOrder, first, count, G->dParent, at, G->hasBind ? (const float*)G->dBind : nullptr, G->dW, records, st));
    }
    return 0;
}
int rigRun(pt_rig* G, const float* at, float* records) { return rigRunLevels(G, at, records, 0, G->plan.levels()); }

// include/pt_rig_ik.h's stage up to the solve (the rig has joints and ikActive()): the locals at `at` brought into dLocals unless they lie
// there, the levels ahead of the solve, and k_rig_ik in place on dLocals
int rigIkSolve(pt_rig* G, const float* at) {
    const hipStream_t st = G->pose->plan->stream;
    if (at != (const float*)G->dLocals) HIP_TRY(hipMemcpyAsync(G->dLocals, at, (size_t)G->n * JOINT_BYTES, hipMemcpyDeviceToDevice, st));
    if (const int rc = rigRunLevels(G, G->dLocals, G->dR, 0, G->ikWindow.before)) return rc;
    HIP_TRY(ptRigIkLaunch(G->dIkRows, G->dIkCons, G->dIkGoals, (int)G->nIk, G->dW, G->dLocals, G->dLocals, st));
    return 0;
}

// the levels of a tail over the locals at `at`: all of them, or with goals set the stage of include/pt_rig_ik.h
int rigLevels(pt_rig* G, const float* at, float* records) {
    if (!G->ikActive()) return rigRun(G, at, records);
    if (const int rc = rigIkSolve(G, at)) return rc;
    return rigRunLevels(G, G->dLocals, records, G->ikWindow.from, G->plan.levels());
}

// the records of the locals at `at` (a source's answer) into dR, and downloaded; the plan's stream is idle afterwards
int rigRecords(pt_rig* G, const float* at, float* out) {
    const hipStream_t st = G->pose->plan->stream;
    if (!at) return PT_ERR_HIP;
    if (G->n) {
        if (const int rc = rigLevels(G, at, G->dR)) return rc;
        HIP_TRY(hipMemcpyAsync(out, G->dR, (size_t)G->n * RECORD_BYTES, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// the same, the download being for the accepted state and the slow paths; then the pose's one path with dR as the records on the device
int rigGeometry(pt_ctx* c, pt_rig* G, const float* at, const float* ellip, size_t ellipBytes, double* rootCost, int* inPlace, const char* who) {
    std::vector<float> R((size_t)G->n * PT_POSE_RECORD_FLOATS);
    if (const int rc = rigRecords(G, at, R.data())) return rc;
    return poseGeometry(c, G->pose, R.data(), R.size() * 4, G->n ? (const float*)G->dR : nullptr, ellip, ellipBytes, rootCost, inPlace, who);
}

}  // namespace

// ---- include/pt_rig.h

int pt_rig_create(pt_pose* P, const int32_t* parent, size_t parentBytes, const float* invBind, size_t bindBytes, pt_rig** out) {
    const bool live = poseLive(P);
    if (int rc = fail(ptp::checkRigCreate(P, live, parent, parentBytes, invBind, bindBytes, out, live ? P->nParts : 0))) return rc;
    pt_rig* G = new pt_rig();
    G->pose = P; G->n = P->nParts; G->hasBind = invBind != nullptr;
    G->parent.assign(parent, parent + G->n);
    ptp::rigPlan(parent, (size_t)G->n, G->plan);
    const hipStream_t st = P->plan->stream;
    const size_t n = (size_t)G->n;
    auto upload = [&]() {
        HIP_TRY(hipSetDevice(P->device));
        HIP_TRY(G->dOrder.upload(G->plan.order.data(), n * 4, st));
        HIP_TRY(G->dParent.upload(parent, n * 4, st));
        HIP_TRY(G->dBind.upload(invBind, invBind ? n * JOINT_BYTES : 0, st));
        HIP_TRY(G->dLocals.reset(atLeast16(n * JOINT_BYTES)));
        HIP_TRY(G->dW.reset(atLeast16(n * JOINT_BYTES)));
        HIP_TRY(G->dR.reset(atLeast16(n * RECORD_BYTES)));
        HIP_TRY(hipStreamSynchronize(st));
        return 0;
    };
    if (const int rc = upload()) { const std::string msg = g_err; delete G; return fail(rc, msg); }
    { std::lock_guard<std::mutex> g(g_posesMutex); g_rigs.insert(G); }
    P->rigs.push_back(G);
    *out = G;
    return PT_OK;
}

int pt_rig_records(pt_rig* G, const float* locals, size_t localBytes, float* recordsOut, size_t recordBytes) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigRecords(live, locals, localBytes, recordsOut, recordBytes, live ? G->n : 0))) return rc;
    return rigRecords(G, localsFromCaller(G, locals), recordsOut);
}

int pt_rig_clip_attach(pt_rig* G, int nKeys, const float* times, size_t timeBytes, const float* values, size_t valueBytes) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigClipAttach(live, nKeys, times, timeBytes, values, valueBytes, live ? G->n : 0))) return rc;
    if (const int rc = rigStore(G, values, valueBytes, G->clip.dKeys)) return rc;
    G->clip.times.assign(times, times + nKeys);
    return PT_OK;
}

int pt_rig_clip_records(pt_rig* G, float t, float* recordsOut, size_t recordBytes) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigClipRecords(live, live && G->clip.nKeys() > 0, t, recordsOut, recordBytes, live ? G->n : 0))) return rc;
    return rigRecords(G, localsFromClip(G, t), recordsOut);
}

int pt_rig_pose_geometry(pt_ctx* c, pt_rig* G, const float* locals, size_t localBytes, const float* ellip, size_t ellipBytes, double* rootCost, int* inPlace) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigGeometry(false, c, live, live && G->pose->ctx == c, locals, localBytes, false, 0.0f, live ? G->n : 0, ellip, ellipBytes))) return rc;
    if (G->pose->stale) return staleRefused("pt_rig_pose_geometry");      // (ahead of the source: a refused call enqueues nothing)
    return rigGeometry(c, G, localsFromCaller(G, locals), ellip, ellipBytes, rootCost, inPlace, "pt_rig_pose_geometry");
}

int pt_rig_clip_pose_geometry(pt_ctx* c, pt_rig* G, float t, const float* ellip, size_t ellipBytes, double* rootCost, int* inPlace) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigGeometry(true, c, live, live && G->pose->ctx == c, nullptr, 0, live && G->clip.nKeys() > 0, t, live ? G->n : 0, ellip, ellipBytes))) return rc;
    if (G->pose->stale) return staleRefused("pt_rig_clip_pose_geometry");
    return rigGeometry(c, G, localsFromClip(G, t), ellip, ellipBytes, rootCost, inPlace, "pt_rig_clip_pose_geometry");
}

void pt_rig_destroy(pt_rig* G) {
    if (!G) return;
    {
        std::lock_guard<std::mutex> g(g_posesMutex);
        if (!g_rigs.erase(G)) return;                             // not a live rig: destroyed already, by this call or with its pose
    }
    pt_pose* P = G->pose;
    hipSetDevice(P->device);
    P->rigs.erase(std::remove(P->rigs.begin(), P->rigs.end(), G), P->rigs.end());
    delete G;
}

// ---- include/pt_rig_mix.h

int pt_rig_mix_clip(pt_rig* G, int slot, int nKeys, const float* times, size_t timeBytes, const float* values, size_t valueBytes) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigMixClip(live, slot, nKeys, times, timeBytes, values, valueBytes, live ? G->n : 0))) return rc;
    if (const int rc = rigStore(G, values, valueBytes, G->mixClip[slot].dKeys)) return rc;
    G->mixClip[slot].times.assign(times, times + nKeys);
    G->slots.nKeys[slot] = nKeys;
    return PT_OK;
}

int pt_rig_mix_mask(pt_rig* G, int slot, const float* weights, size_t weightBytes) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigMixMask(live, slot, weights, weightBytes, live ? G->n : 0))) return rc;
    if (const int rc = rigStore(G, weights, weightBytes, G->dMixMask[slot])) return rc;
    G->slots.mask[slot] = true;
    return PT_OK;
}

int pt_rig_mix_locals(pt_rig* G, const pt_rig_layer* layers, size_t layerBytes, float* localsOut, size_t localBytes) {
    if (int rc = mixRefused(ptp::RIG_MIX_LOCALS, nullptr, G, layers, layerBytes, localsOut, localBytes)) return rc;
    const hipStream_t st = G->pose->plan->stream;
    const float* at = localsFromMix(G, rigMixTable(G, layers, layerBytes));
    if (!at) return PT_ERR_HIP;
    if (G->n) HIP_TRY(hipMemcpyAsync(localsOut, at, localBytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PT_OK;
}

int pt_rig_mix_records(pt_rig* G, const pt_rig_layer* layers, size_t layerBytes, float* recordsOut, size_t recordBytes) {
    if (int rc = mixRefused(ptp::RIG_MIX_RECORDS, nullptr, G, layers, layerBytes, recordsOut, recordBytes)) return rc;
    return rigRecords(G, localsFromMix(G, rigMixTable(G, layers, layerBytes)), recordsOut);
}

int pt_rig_mix_pose_geometry(pt_ctx* c, pt_rig* G, const pt_rig_layer* layers, size_t layerBytes, const float* ellip, size_t ellipBytes, double* rootCost, int* inPlace) {
    if (int rc = mixRefused(ptp::RIG_MIX_GEOMETRY, c, G, layers, layerBytes, ellip, ellipBytes)) return rc;
    if (G->pose->stale) return staleRefused("pt_rig_mix_pose_geometry");
    return rigGeometry(c, G, localsFromMix(G, rigMixTable(G, layers, layerBytes)), ellip, ellipBytes, rootCost, inPlace, "pt_rig_mix_pose_geometry");
}

// ---- include/pt_rig_ik.h

int pt_rig_ik_attach(pt_rig* G, const pt_rig_ik_constraint* cons, size_t bytes) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigIkAttach(live, cons, bytes, live ? G->parent.data() : nullptr, live ? G->n : 0))) return rc;
    const size_t n = bytes / sizeof(pt_rig_ik_constraint);
    std::vector<ptp::RigIkRow> rows(n);
    for (size_t k = 0; k < n; k++) rows[k] = ptp::rigIkRow(G->parent.data(), cons[k]);
    Dev<int32_t> dRows;
    Dev<float> dCons;
    if (const int rc = rigStore(G, rows.data(), n * sizeof(ptp::RigIkRow), dRows)) return rc;
    if (const int rc = rigStore(G, cons, bytes, dCons)) return rc;
    G->dIkRows = std::move(dRows); G->dIkCons = std::move(dCons);     // (both stand: the rig changes now)
    G->nIk = n;
    G->ikWindow = ptp::rigIkWindow(G->parent.data(), (size_t)G->n, cons, n);
    G->ikGoals = false;
    G->dIkGoals.release();
    return PT_OK;
}

int pt_rig_ik_goals(pt_rig* G, const pt_rig_ik_goal* goals, size_t bytes) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigIkGoals(live, goals, bytes, live ? G->nIk : 0))) return rc;
    if (!goals) { G->ikGoals = false; return PT_OK; }
    if (const int rc = rigStore(G, goals, bytes, G->dIkGoals)) return rc;
    G->ikGoals = true;
    return PT_OK;
}

int pt_rig_ik_locals(pt_rig* G, const float* locals, size_t localBytes, float* localsOut, size_t outBytes) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigIkLocals(live, locals, localBytes, localsOut, outBytes, live ? G->n : 0))) return rc;
    const hipStream_t st = G->pose->plan->stream;
    const float* at = localsFromCaller(G, locals);
    if (!at) return PT_ERR_HIP;
    if (G->n) {
        if (G->ikActive())
            if (const int rc = rigIkSolve(G, at)) return rc;
        HIP_TRY(hipMemcpyAsync(localsOut, G->dLocals, outBytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return PT_OK;
}
