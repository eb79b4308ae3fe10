// pt_pose_host.hpp — the host half of include/pt_pose.h behind the C ABI (included at the end of pt_image.hpp after pt_move_host.hpp, inside
// pt_hip.hip's extern "C" block, where pt_ctx, the in-place move and their helpers are in scope; not a translation unit).  The kernels are
// pt_pose.hip's, behind pt_pose_launch.hpp; the refit is pt_refit.hip's second half (pt_refit_kernels_); the patch of the context's records is
// pt_move_host.hpp's (movePatchRecords), fed from the rows of binding 10 that k_pose_gather collects; the argument checks and the CPU statement
// of the rule are pt_pose_rule.hpp's.  A skinned pose (include/pt_skin.h, pt_skin_create) is the same object under a second rule: its two corner
// tables instead of the part ids, pt_skin.hip's kernel behind pt_skin_launch.hpp instead of k_pose, pt_skin_rule.hpp's checks; ruleLaunch is
// the one place that tells them apart.  A morph (include/pt_morph.h, pt_morph_attach) belongs to either kind: pt_morph.hip's kernel behind
// pt_morph_launch.hpp writes the morphed copy of the rest pose's affected corners, which poseInto hands to the pose's rule in place of dRest;
// pt_morph_rule.hpp's checks and inverted index.  Normals (include/pt_normals.h, pt_normals_attach) belong to either kind too: pt_normals.hip's
// two launches behind pt_normals_launch.hpp recompute the normals of the welded corners at the end of poseInto, from what the pose's rule wrote;
// pt_normals_rule.hpp's checks and inverted index.  A DQ pose (include/pt_skin_dq.h, pt_skin_dq_create) is a skinned pose under a third rule: the same two
// corner tables, pt_skin_dq.hip's two launches behind pt_skin_dq_launch.hpp (the records into dDq, a table the pose owns, then the corners)
// instead of pt_skin.hip's one, pt_skin_dq_rule.hpp's CPU statement; again ruleLaunch is the one place that tells them apart.
//
// One of each: ruleLaunch launches the pose's rule (pt_pose::rule says which of the three), for poseInto with the statements chosen below and for
// the debug timers with the caller's; bestTime is the one timing loop of the six pt_debug_*_time calls; poseAccepted records a call's records,
// weights and normals mode as the pose's last accepted state (PoseState), which a refused call hands back to poseInto.
//
// A rig (include/pt_rig.h, pt_rig_create) belongs to a pose of any rule and makes that pose's records on the device: pt_rig.hip's launches behind
// pt_rig_launch.hpp (the key blend, then one launch per level of the hierarchy) write them into the rig's dR, pt_rig_rule.hpp's checks, level
// plan, clip interval and CPU statement.  poseGeometry is pt_pose_geometry after its argument checks, for the pose's own call and for the rig's
// calls: with the records also lying on the device, poseInto copies them from there into dX instead of uploading them, and nothing else differs.
// A mix (include/pt_rig_mix.h) is a third source of a rig's locals beside the caller's and the clip's: pt_rig_mix.hip's one launch behind
// pt_rig_mix_launch.hpp writes them into dLocals from the rig's clip and mask slots, pt_rig_mix_rule.hpp's checks, loop wrap and CPU statement.
//
// What the pose's plan holds.  plan->dTris: static triangles (part -1) are the rest pose's from creation on and are never written again by a
// kernel (the slow path's upload writes the same values); the others hold the pose last run.  While the context is behind on this pose
// (c->behind == pose), dTris and dData are the bindings 3 and 10 a settle delivers: a refused pose is undone by running the last accepted one again.
extern "C++" {
#include "pt_pose_launch.hpp"
#include "pt_pose_rule.hpp"
#include "pt_skin_launch.hpp"
#include "pt_skin_rule.hpp"
#include "pt_skin_dq_launch.hpp"
#include "pt_skin_dq_rule.hpp"
#include "pt_morph_launch.hpp"
#include "pt_morph_rule.hpp"
#include "pt_normals_launch.hpp"
#include "pt_normals_rule.hpp"
#include "pt_rig_launch.hpp"
#include "pt_rig_mix_launch.hpp"
#include "pt_rig_mix_rule.hpp"
#include "pt_rig_rule.hpp"
#include <set>
}
#include "../../../include/pt_pose.h"
#include "../../../include/pt_skin.h"
#include "../../../include/pt_skin_dq.h"
#include "../../../include/pt_morph.h"
#include "../../../include/pt_normals.h"
#include "../../../include/pt_rig.h"
#include "../../../include/pt_rig_mix.h"

// the rule of a pose: per-part matrices from dPart (include/pt_pose.h); records blended per corner from dBone / dWeight, 12 words per triangle and
// no dPart (include/pt_skin.h); the same two tables under the dual-quaternion blend (include/pt_skin_dq.h)
enum PoseRule { RULE_PARTS, RULE_SKIN, RULE_SKIN_DQ };

// what a pose call is asked for, and what is kept of the last accepted one
struct PoseState {
    std::vector<float> xforms;          // the records; empty: none accepted yet (the rest pose, unmorphed, its normals as they are), or n_parts == 0
    std::vector<float> weights;         // the morph weights; empty: every weight 0 (none accepted yet, or accepted before the attach)
    int mode = 0;                       // the normals mode (none accepted yet, or accepted before the attach: 0)
};

struct pt_pose {
    pt_ctx* ctx = nullptr;              // the context (a group's: the group) it was created on and belongs to
    int device = 0, nParts = 0; int64_t nTris = 0;
    pt_refit_plan* plan = nullptr;      // its own, over the context's bindings 10-13
    Dev<float> dRest, dScratch, dX, dRows; Dev<int32_t> dPart, dRowIds;
    PoseRule rule = RULE_PARTS;
    Dev<int32_t> dBone; Dev<float> dWeight;
    Dev<float> dDq;                     // RULE_SKIN_DQ: the dual quaternions of the records, 32 bytes each
    bool scratchReady = false;          // dScratch holds the rest pose's static triangles (pt_pose_triangles, the slow paths)
    int rowsFor = -1, nRows = 0;        // dRowIds lists the rows of the plan's map made under this bfs_nodes
    PoseState accepted;                 // the last accepted pose: a refused call is undone by running it again
    // include/pt_morph.h: nTargets > 0 once a morph is attached.  dMorphRest is a second copy of the rest pose, of which the kernel rewrites the
    // affected corners (all of them, on every morphed call) and nothing else
    int nTargets = 0; int64_t nAffected = 0;
    Dev<float> dMorphRest, dMorphW; Dev<int32_t> dMorphCorner, dMorphRow; Dev<ptp::MorphEntry> dMorphEntry;
    std::vector<float> weights;         // as pt_morph_weights set them last (after the attach: zeros)
    // include/pt_normals.h: hasNormals once normals are attached.  The inverted index of pt_normals_rule.hpp (the listed triangles, the row starts
    // of the non-empty vertices, their corners, per corner its row) and the face vectors, 16 bytes per triangle, indexed by triangle id
    bool hasNormals = false; uint32_t normalsFlags = 0;
    int64_t nNrmTris = 0, nNrmRows = 0, nNrmCorners = 0;
    Dev<int32_t> dNrmTri, dNrmRow, dNrmCorner, dNrmCornerRow; Dev<float> dNrmFace;
    int normalsMode = 0;                // as pt_normals_mode set it last (after the attach: 1)
    bool stale = false;                 // the scene was uploaded since pt_pose_create
    std::vector<pt_rig*> rigs;          // include/pt_rig.h: the rigs attached to this pose, which go with it
};

// a rig of include/pt_rig.h: one joint per record of its pose
struct pt_rig {
    pt_pose* pose = nullptr;
    int n = 0;                          // joints == the pose's n_parts
    ptp::RigPlan plan;                  // the joints by (depth, id) and the level starts
    bool hasBind = false;
    Dev<int32_t> dOrder, dParent;       // the plan's order; the parents by joint id
    Dev<float> dBind, dLocals, dW, dR;  // 12 floats per joint: the inverse binds, the locals of a call (or a clip's blend), the world matrices; the records, 24 per joint
    int nKeys = 0;                      // include/pt_rig.h step 5: > 0 once a clip is attached
    std::vector<float> times;
    Dev<float> dClip;                   // n_keys * n locals, key-major
    // include/pt_rig_mix.h: the clip slots (as the clip above, per slot; slots.nKeys[i] > 0 once slot i is filled) and the mask slots, n floats each
    ptp::RigMixSlots slots;
    std::vector<float> mixTimes[PT_RIG_MIX_SLOTS];
    Dev<float> dMixClip[PT_RIG_MIX_SLOTS], dMixMask[PT_RIG_MIX_MASKS];
};

namespace {

std::mutex g_posesMutex;
std::set<pt_pose*> g_poses;             // the live poses: a destroyed one is refused, not followed
constexpr PtPoseKernel POSE_KERNEL = PT_POSE_PER_QUAD;      // the faster of the two at 100 k and at 1 M triangles (scripts/pose_probe.py); pt_debug_pose_time runs either
constexpr PtNormalsKernel NORMALS_KERNEL = PT_NORMALS_PER_CORNER;   // 5 % slower on C4's mesh, 10 % faster on the 1 M height field: the shorter summed over both (71.9 against 77.4 us), and twice as fast on a table with one long row (scripts/normals_probe.py); pt_debug_normals_time runs either
constexpr PtSkinKernel SKIN_KERNEL = PT_SKIN_PER_CORNER;    // faster with four slots at 100 k and at 1 M triangles, tied at 100 k and 2 % slower at 1 M with two: the shorter summed over both slot counts at 1 M (scripts/skin_probe.py); pt_debug_skin_time runs either
constexpr int RULE_KERNEL[3] = {POSE_KERNEL, SKIN_KERNEL, 0};    // by PoseRule: the statement poseInto runs (the DQ rule has one)

bool poseLive(pt_pose* p) {
    std::lock_guard<std::mutex> g(g_posesMutex);
    return p && g_poses.count(p);
}

std::set<pt_rig*> g_rigs;               // the live rigs, under g_posesMutex: a rig leaves with its pose at the latest
bool rigLive(pt_rig* r) {
    std::lock_guard<std::mutex> g(g_posesMutex);
    return r && g_rigs.count(r);
}

// the morphed rest pose under `weights` (host, nTargets floats) into dMorphRest; asynchronous on the plan's stream
int morphRest(pt_pose* P, const float* weights) {
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipMemcpyAsync(P->dMorphW, weights, (size_t)P->nTargets * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ptMorphLaunch(P->dRest, P->dMorphCorner, P->dMorphRow, P->dMorphEntry, P->dMorphW, P->nAffected, P->dMorphRest, st));
    return 0;
}

// the normals of dst's welded corners from dst's vertices, by the statement `which` of the gather; asynchronous on the plan's stream
int normalsInto(pt_pose* P, float* dst, PtNormalsKernel which) {
    const hipStream_t st = P->plan->stream;
    HIP_TRY(ptNormalsFacesLaunch(dst, P->dNrmTri, P->nNrmTris, (P->normalsFlags & PT_NORMALS_FLIP) != 0, P->dNrmFace, st));
    HIP_TRY(ptNormalsGatherLaunch(P->dNrmFace, P->dNrmRow, P->nNrmRows, P->dNrmCorner, P->dNrmCornerRow, P->nNrmCorners, dst, which, st));
    return 0;
}

bool hasBones(const pt_pose* P) { return P->rule != RULE_PARTS; }        // dBone / dWeight instead of dPart

// the pose's rule from `rest` into dst, over the records that lie in dX, by the statement `which` of its kernel (a PtPoseKernel or a PtSkinKernel;
// the DQ rule has one statement: the records into dDq, then the corners); asynchronous on the plan's stream
hipError_t ruleLaunch(pt_pose* P, const float* rest, float* dst, int which) {
    const hipStream_t st = P->plan->stream;
    switch (P->rule) {
        case RULE_PARTS: return ptPoseLaunch(rest, P->dPart, P->nTris, P->dX, dst, (PtPoseKernel)which, st);
        case RULE_SKIN: return ptSkinLaunch(rest, P->dBone, P->dWeight, P->nTris, P->dX, dst, (PtSkinKernel)which, st);
        case RULE_SKIN_DQ: {
            const hipError_t e = ptSkinDqRecordsLaunch(P->dX, P->nParts, P->dDq, st);
            return e != hipSuccess ? e : ptSkinDqLaunch(rest, P->dBone, P->dWeight, P->nTris, P->dDq, dst, st);
        }
    }
    return hipErrorInvalidValue;
}

// the pose of `xforms` (host; nullptr: the rest pose, unmorphed, its normals as they are) under the morph weights `weights` (host; empty: no morph,
// or every weight 0) and the normals mode `mode` (1: recomputed where normals are attached) into dst, which holds the rest pose's static
// triangles; asynchronous on the plan's stream.  onDevice: where the same records lie on the device already (a rig's dR): copied from there,
// not uploaded
int poseInto(pt_pose* P, const float* xforms, const std::vector<float>& weights, int mode, float* dst, const float* onDevice = nullptr) {
    const hipStream_t st = P->plan->stream;
    if (!xforms || P->nParts == 0) {                              // (n_parts == 0: a morph has no entries)
        if (P->nTris) HIP_TRY(hipMemcpyAsync(dst, P->dRest, (size_t)P->nTris * 160, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    // every weight +-0: the morphed rest pose is the rest pose, bit for bit (the header's consequence 1), and the launch is skipped
    bool morphed = false;
    for (const float w : weights) morphed = morphed || w != 0.0f;
    if (morphed) { if (const int rc = morphRest(P, weights.data())) return rc; }
    const float* rest = morphed ? (const float*)P->dMorphRest : (const float*)P->dRest;
    HIP_TRY(P->dX.ensure((size_t)P->nParts * 96));
    if (onDevice) HIP_TRY(hipMemcpyAsync(P->dX, onDevice, (size_t)P->nParts * 96, hipMemcpyDeviceToDevice, st));
    else HIP_TRY(hipMemcpyAsync(P->dX, xforms, (size_t)P->nParts * 96, hipMemcpyHostToDevice, st));
    HIP_TRY(ruleLaunch(P, rest, dst, RULE_KERNEL[P->rule]));
    if (P->hasNormals && mode == 1) return normalsInto(P, dst, NORMALS_KERNEL);
    return 0;
}
// poseInto of a kept state: the one place that reads what its empty fields mean
int poseStateInto(pt_pose* P, const PoseState& s, float* dst) { return poseInto(P, s.xforms.empty() ? nullptr : s.xforms.data(), s.weights, s.mode, dst); }

// what this call was asked for is the pose's last accepted state
void poseAccepted(pt_pose* P, const float* xforms, size_t xformBytes) {
    P->accepted.xforms.assign(xforms, xforms + xformBytes / 4);
    P->accepted.weights = P->weights;
    P->accepted.mode = P->normalsMode;
}

// P = the rule applied to the rest pose, on the host; the plan's working copies are not touched
int poseToHost(pt_pose* P, const float* xforms, const std::vector<float>& weights, int mode, float* out) {
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipSetDevice(P->device));
    if (!P->scratchReady) {
        HIP_TRY(P->dScratch.reset(P->nTris ? (size_t)P->nTris * 160 : 16));
        if (P->nTris) HIP_TRY(hipMemcpyAsync(P->dScratch, P->dRest, (size_t)P->nTris * 160, hipMemcpyDeviceToDevice, st));
        P->scratchReady = true;
    }
    if (const int rc = poseInto(P, xforms, weights, mode, P->dScratch)) return rc;
    if (P->nTris) HIP_TRY(hipMemcpyAsync(out, P->dScratch, (size_t)P->nTris * 160, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// the scratch copy holds the whole rest pose again, the records `xforms` lie in dX and the plan's stream is idle: what pt_debug_pose_scratch reads
// after a launch of the pose's rule into the scratch copy is that launch's work alone
int scratchAtRest(pt_pose* P, const float* xforms) {
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipSetDevice(P->device));
    if (!P->scratchReady) HIP_TRY(P->dScratch.reset(P->nTris ? (size_t)P->nTris * 160 : 16));
    if (P->nTris) HIP_TRY(hipMemcpyAsync(P->dScratch, P->dRest, (size_t)P->nTris * 160, hipMemcpyDeviceToDevice, st));
    P->scratchReady = true;
    HIP_TRY(P->dX.ensure((size_t)P->nParts * 96));
    HIP_TRY(hipMemcpyAsync(P->dX, xforms, (size_t)P->nParts * 96, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// THE timing loop of include/pt_debug.h: the device time between a pair of events on `st` around what `enqueue` puts there (false: it could not),
// the best of reps, into *msBest — which a failure leaves as it was.  The events are destroyed on every path
extern "C++" template <class Enqueue>
int bestTime(hipStream_t st, int reps, const char* who, Enqueue enqueue, float* msBest) {
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); }
    } ev;
    hipEvent_t &e0 = ev.e0, &e1 = ev.e1;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
    float best = 0.0f;
    for (int k = 0; k < reps; k++) {
        hipEventRecord(e0, st);
        const bool enqueued = enqueue();
        hipEventRecord(e1, st);
        float ms = 0.0f;
        if (!enqueued || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return fail(PT_ERR_HIP, std::string(who) + ": the launch failed");
        if (k == 0 || ms < best) best = ms;
    }
    *msBest = best;
    return 0;
}

// the three rule timers after their checks: the statement `which` of the pose's rule from the rest pose into the scratch copy
int ruleTime(pt_pose* P, const float* xforms, int which, int reps, const char* who, float* msBest) {
    if (const int rc = scratchAtRest(P, xforms)) return rc;
    return bestTime(P->plan->stream, reps, who, [&] { return ruleLaunch(P, P->dRest, P->dScratch, which) == hipSuccess; }, msBest);
}

// which corners the pose's rule moves, a byte per corner: from the part ids or the bone table, which lie on the device (no triangles: left empty)
int movedCorners(pt_pose* P, std::vector<unsigned char>& moved) {
    if (!P->nTris) return 0;
    const hipStream_t st = P->plan->stream;
    const bool bones = hasBones(P);
    HIP_TRY(hipSetDevice(P->device));
    moved.resize((size_t)P->nTris * 3);
    std::vector<int32_t> words((size_t)P->nTris * (bones ? 12 : 1));
    HIP_TRY(hipMemcpyAsync(words.data(), bones ? P->dBone : P->dPart, words.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t q = 0; q < moved.size(); q++) moved[q] = (bones ? words[4 * q] : words[q / 3]) >= 0;
    return 0;
}

void poseFree(pt_pose* P) {
    hipSetDevice(P->device);
    {
        std::lock_guard<std::mutex> g(g_posesMutex);
        for (pt_rig* r : P->rigs) g_rigs.erase(r);
    }
    for (pt_rig* r : P->rigs) delete r;
    pt_refit_destroy(P->plan);
    delete P;
}

// ---- what pt_context.hpp declares

int settleScene(pt_ctx* c) {
    pt_pose* P = c->behind;
    if (!P) return 0;
    pt_refit_plan* plan = P->plan;
    HIP_TRY(hipSetDevice(c->device));
    c->buf.tris.resize((size_t)P->nTris * 40);
    c->buf.bvhdata.resize(plan->dataBytes / 4);
    if (P->nTris) HIP_TRY(hipMemcpyAsync(c->buf.tris.data(), plan->dTris, (size_t)P->nTris * 160, hipMemcpyDeviceToHost, plan->stream));
    if (plan->dataBytes) HIP_TRY(hipMemcpyAsync(c->buf.bvhdata.data(), plan->dData, plan->dataBytes, hipMemcpyDeviceToHost, plan->stream));
    HIP_TRY(hipStreamSynchronize(plan->stream));
    c->behind = nullptr;
    return 0;
}

int poseMotionRecords(pt_ctx* on, const float4* then, int nThen, Dev<float4>& out, int* nTri) {
    const pt_pose* P = on->behind;                                // (its plan's stream is idle: every pose call ends synchronised)
    const int n = (int)P->nTris;
    HIP_TRY(hipSetDevice(on->device));
    HIP_TRY(out.ensure(std::max<size_t>((size_t)n * 48, 16)));    // (kept from call to call: the count cannot change while the context is behind)
    if (n == 0) HIP_TRY(hipMemsetAsync(out, 0, 16, on->stream)); // (motionPack's one zero record)
    HIP_TRY(ptPoseMotionLaunch(P->plan->dTris, n, then, nThen, out, on->stream));
    *nTri = n;
    return 0;
}

int markPositionsToHost(pt_ctx* on) {
    pt_ctx::Mark& m = on->mark;
    std::vector<float> recs((size_t)m.nTri * 12);
    HIP_TRY(hipSetDevice(on->device));
    if (m.nTri) HIP_TRY(hipMemcpyAsync(recs.data(), m.dTri, recs.size() * 4, hipMemcpyDeviceToHost, on->stream));
    HIP_TRY(hipStreamSynchronize(on->stream));
    m.tri.resize((size_t)m.nTri * 9);
    for (size_t t = 0; t < (size_t)m.nTri; t++)
        for (int v = 0; v < 3; v++) std::memcpy(&m.tri[9 * t + 3 * v], &recs[12 * t + 4 * v], 12);
    m.triOnDevice = false;
    return 0;
}

void posesStale(pt_ctx* c) { for (pt_pose* p : c->poses) p->stale = true; }

void posesDestroy(pt_ctx* c) {
    c->behind = nullptr;                                          // (nobody will read the host copies again)
    for (pt_pose* p : c->poses) {
        { std::lock_guard<std::mutex> g(g_posesMutex); g_poses.erase(p); }
        poseFree(p);
    }
    c->poses.clear();
}

// the slow paths: P on the host, then pt_move_geometry's own sequence with the pose's plan
int poseSlow(pt_ctx* c, pt_pose* P, const float* xforms, size_t xformBytes, const float* ellip, size_t ellipBytes, double* rootCost, int* inPlace) {
    int rc;
    if (!c->multi && (rc = settleScene(c))) return rc;            // (the move uploads into the plan's working copy)
    std::vector<float> tris((size_t)P->nTris * 40);
    if ((rc = poseToHost(P, xforms, P->weights, P->normalsMode, tris.data()))) return rc;
    // (a group's sequence goes through pt_set_buffer, which marks the context's poses stale: these uploads are the pose's own — binding 3 is the rule
    //  applied to the rest pose, the trees are the plan's — so every pose stays what it was, as on the in-place path)
    std::vector<char> was;
    for (const pt_pose* p : c->poses) was.push_back(p->stale);
    rc = moveGeometry(c, P->plan, tris.data(), tris.size() * 4, ellip, ellipBytes, rootCost, inPlace);
    for (size_t k = 0; k < was.size(); k++) c->poses[k]->stale = was[k] != 0;
    if (rc) return rc;
    poseAccepted(P, xforms, xformBytes);
    return PT_OK;
}

// pt_pose_create, pt_skin_create and pt_skin_dq_create after their argument checks: triPart under RULE_PARTS, the two corner tables of a skin
// under the other two
int poseCreate(pt_ctx* c, size_t nTris, int nParts, PoseRule rule, const int32_t* triPart, const int32_t* bone, const float* weight, pt_pose** out) {
    int rc;
    if (c->multi) {
        if (!c->multi->staleBindings.empty()) return fail(PT_ERR_SCENE, MULTI_UPLOAD_FAILED);
        if ((rc = multiFlushAndBuild(*c->multi))) return rc;
    } else {
        HIP_TRY(hipSetDevice(c->device));
        if ((rc = flushStream(c))) return rc;
        if (c->sceneDirty && (rc = buildScene(c))) return rc;
    }
    pt_ctx* on = firstStream(c);
    SceneBuffers* host = nullptr;
    if ((rc = settledScene(on, &host))) return rc;
    const SceneBuffers& b = *host;
    pt_refit_plan* plan = nullptr;
    if ((rc = pt_refit_create(on->device, b.bvhdata.data(), b.bvhdata.size() * 4, b.bvhtree.data(), b.bvhtree.size() * 4, b.leaftris.data(), b.leaftris.size() * 4,
                              b.objidx.data(), b.objidx.size() * 4, (int64_t)nTris, &plan)))
        return rc;
    pt_pose* P = new pt_pose();
    P->ctx = c; P->device = on->device; P->nParts = nParts; P->nTris = (int64_t)nTris; P->plan = plan; P->rule = rule;
    const hipStream_t st = plan->stream;
    auto upload = [&]() {
        HIP_TRY(hipSetDevice(P->device));
        HIP_TRY(P->dRest.upload(b.tris.data(), nTris * 160, st));
        if (hasBones(P)) {
            HIP_TRY(P->dBone.upload(bone, nTris * 48, st));
            HIP_TRY(P->dWeight.upload(weight, nTris * 48, st));
        } else HIP_TRY(P->dPart.upload(triPart, nTris * 4, st));
        HIP_TRY(P->dX.reset(std::max<size_t>((size_t)nParts * 96, 16)));
        if (rule == RULE_SKIN_DQ) HIP_TRY(P->dDq.reset(std::max<size_t>((size_t)nParts * 32, 16)));
        if (nTris) HIP_TRY(hipMemcpyAsync(plan->dTris, P->dRest, nTris * 160, hipMemcpyDeviceToDevice, st));      // the static triangles, once
        HIP_TRY(hipStreamSynchronize(st));
        return 0;
    };
    if ((rc = upload())) { const std::string msg = g_err; poseFree(P); return fail(rc, msg); }
    { std::lock_guard<std::mutex> g(g_posesMutex); g_poses.insert(P); }
    c->poses.push_back(P);
    *out = P;
    return PT_OK;
}

}  // namespace

int pt_pose_create(pt_ctx* c, const int32_t* triPart, size_t partBytes, int nParts, pt_pose** out) {
    const size_t nTris = c ? hostTriangleCount(firstStream(c)) : 0;
    if (int rc = fail(ptp::checkPoseCreate(c, triPart, partBytes, nParts, out, nTris))) return rc;
    return poseCreate(c, nTris, nParts, RULE_PARTS, triPart, nullptr, nullptr, out);
}

int pt_skin_create(pt_ctx* c, const int32_t* bone, size_t boneBytes, const float* weight, size_t weightBytes, int nParts, pt_pose** out) {
    const size_t nTris = c && bone && weight && out ? hostTriangleCount(firstStream(c)) : 0;     // (the context is read only once no argument is null)
    if (int rc = fail(ptp::checkSkinCreate(c, bone, boneBytes, weight, weightBytes, nParts, out, nTris))) return rc;
    return poseCreate(c, nTris, nParts, RULE_SKIN, nullptr, bone, weight, out);
}

int pt_skin_dq_create(pt_ctx* c, const int32_t* bone, size_t boneBytes, const float* weight, size_t weightBytes, int nParts, pt_pose** out) {
    const size_t nTris = c && bone && weight && out ? hostTriangleCount(firstStream(c)) : 0;     // (the context is read only once no argument is null)
    if (int rc = fail(ptp::checkSkinCreate(c, bone, boneBytes, weight, weightBytes, nParts, out, nTris, nullptr, "pt_skin_dq_create"))) return rc;
    return poseCreate(c, nTris, nParts, RULE_SKIN_DQ, nullptr, bone, weight, out);
}

int pt_pose_triangles(pt_pose* P, const float* xforms, size_t xformBytes, float* trisOut, size_t triBytes) {
    const bool live = poseLive(P);
    if (int rc = fail(ptp::checkPoseTriangles(live, xforms, xformBytes, live ? P->nParts : 0, trisOut, triBytes, live ? (size_t)P->nTris : 0))) return rc;
    return poseToHost(P, xforms, P->weights, P->normalsMode, trisOut);
}

namespace {
// pt_pose_geometry after its argument checks, under the name `who` of the call it serves; onDevice: as for poseInto
int poseGeometry(pt_ctx* c, pt_pose* P, const float* xforms, size_t xformBytes, const float* onDevice, const float* ellip, size_t ellipBytes, double* rootCost, int* inPlace,
                 const char* who) {
    if (P->stale) return fail(PT_ERR_SCENE, std::string(who) + ": the scene was uploaded since pt_pose_create");
    if (c->multi) return poseSlow(c, P, xforms, xformBytes, ellip, ellipBytes, rootCost, inPlace);
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = flushStream(c))) return rc;                         // submitted frames are rendered in the old scene
    if (c->sceneDirty && (rc = buildScene(c))) return rc;         // (settles)
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (ellip) { std::string err; if ((rc = ptl::ellipsoidsUsable(ellip, ellipBytes / 4, c->sc.numMat, err))) return fail(rc, err); }
    pt_refit_plan* plan = P->plan;
    if (c->asmWhyNot == MOVE_UNORDERED || (ellip && !ptl::ellipPatchable(c->buf.ellip, ellip, ellipBytes / 4)))
        return poseSlow(c, P, xforms, xformBytes, ellip, ellipBytes, rootCost, inPlace);
    // the map of the record order reads the host copies: made (rarely: the first call, a changed bfs_nodes) before the working copies change
    if (!plan->mapValid || plan->mapBfsNodes != c->opt.bfsNodes) {
        if ((rc = moveEnsureMap(c, plan))) return rc;            // (settles)
    }
    if (!moveMapFits(c, plan)) return poseSlow(c, P, xforms, xformBytes, ellip, ellipBytes, rootCost, inPlace);
    ptl::MoveMap& map = plan->map;
    const hipStream_t ps = plan->stream;
    if (P->rowsFor != plan->mapBfsNodes) {
        std::vector<int32_t> ids;
        ptl::moveRowIds(map, ids);
        HIP_TRY(P->dRowIds.upload(ids.data(), ids.size() * 4, ps));
        HIP_TRY(P->dRows.reset(std::max<size_t>(ids.size() * 32, 16)));
        HIP_TRY(hipStreamSynchronize(ps));
        P->nRows = (int)ids.size(); P->rowsFor = plan->mapBfsNodes;
    }

    // pose + refit: the plan's working copies only.  A refusal puts back what a settle would have delivered
    if (!(rc = poseInto(P, xforms, P->weights, P->normalsMode, plan->dTris, onDevice))) rc = pt_refit_kernels_(plan, who);
    if (rc) {
        const std::string msg = g_err;
        if (c->behind == P) {
            int rc2 = poseStateInto(P, P->accepted, plan->dTris);
            if (!rc2) rc2 = pt_refit_kernels_(plan, who);
            if (rc2) return rc2;
        }
        return fail(rc, msg);
    }
    // the rows the root and group records need, the costs, the root records: the plan's stream is idle afterwards
    std::vector<float> rows((size_t)P->nRows * 8);
    std::vector<double> cost(std::max(plan->s.nRoots, 1));
    std::vector<ObjRoot> roots(c->dRoots.bytes / sizeof(ObjRoot));
    HIP_TRY(ptPoseGatherLaunch(plan->dData, P->dRowIds, P->nRows, P->dRows, ps));
    if (P->nRows) HIP_TRY(hipMemcpyAsync(rows.data(), P->dRows, rows.size() * 4, hipMemcpyDeviceToHost, ps));
    if (plan->s.nRoots > 0) HIP_TRY(hipMemcpyAsync(cost.data(), plan->dRootCost, (size_t)plan->s.nRoots * 8, hipMemcpyDeviceToHost, ps));
    HIP_TRY(hipMemcpyAsync(roots.data(), c->dRoots, roots.size() * sizeof(ObjRoot), hipMemcpyDeviceToHost, ps));
    HIP_TRY(hipStreamSynchronize(ps));

    // ---- the patch: from here on the context's records change
    map.asmStride = c->built.asmNodeStride; map.asmGroupShift = c->asmGroupShift; map.asmNoRootCull = c->opt.asmNoRootCull;
    ptl::moveRootsGathered(map, rows.data(), roots.data());
    int unordered = 0;
    if ((rc = movePatchRecords(c, plan, roots, ellip, &unordered))) return rc;
    c->behind = P;                                                // a pose the context was behind on before is superseded
    poseAccepted(P, xforms, xformBytes);
    bool rebuilt = false;
    if ((rc = moveCommitted(c, ellip, ellipBytes, unordered, &rebuilt))) return rc;       // (a rebuild settles)
    if (rootCost) std::copy(cost.begin(), cost.begin() + plan->s.nRoots, rootCost);
    if (inPlace) *inPlace = rebuilt ? 0 : 1;
    return PT_OK;
}
}  // namespace

int pt_pose_geometry(pt_ctx* c, pt_pose* P, const float* xforms, size_t xformBytes, const float* ellip, size_t ellipBytes, double* rootCost, int* inPlace) {
    const bool live = poseLive(P);
    if (int rc = fail(ptp::checkPoseGeometry(c, live, live && P->ctx == c, xforms, xformBytes, live ? P->nParts : 0, ellip, ellipBytes))) return rc;
    return poseGeometry(c, P, xforms, xformBytes, nullptr, ellip, ellipBytes, rootCost, inPlace, "pt_pose_geometry");
}

void pt_pose_destroy(pt_pose* P) {
    if (!P) return;
    {
        std::lock_guard<std::mutex> g(g_posesMutex);
        if (!g_poses.erase(P)) return;                            // not a live pose: destroyed already, by this call or with its context
    }
    pt_ctx* c = P->ctx;
    if (c->behind == P) settleScene(c);                           // the posed bindings become the host copies they describe
    if (c->behind == P) c->behind = nullptr;                      // (a failed download: the copies stay the last settled ones)
    c->poses.erase(std::remove(c->poses.begin(), c->poses.end(), P), c->poses.end());
    poseFree(P);
}

// include/pt_debug.h: the device time of one pose launch (the best of reps), into the pose's scratch copy
int pt_debug_pose_time(pt_pose* P, const float* xforms, size_t xformBytes, int which, int reps, float* msBest) {
    const bool live = poseLive(P);
    if (!live || !msBest || reps < 1 || (which != PT_POSE_PER_QUAD && which != PT_POSE_PER_TRIANGLE) || !xforms || P->nParts < 1 || xformBytes != (size_t)P->nParts * 96)
        return fail(PT_ERR_ARG, "pt_debug_pose_time: bad argument");
    if (P->rule == RULE_SKIN_DQ) return fail(PT_ERR_ARG, "pt_debug_pose_time: a DQ pose has no part table (pt_debug_skin_dq_time times its kernels)");
    if (P->rule == RULE_SKIN) return fail(PT_ERR_ARG, "pt_debug_pose_time: a skinned pose has no part table (pt_debug_skin_time times its kernels)");
    return ruleTime(P, xforms, which, reps, "pt_debug_pose_time", msBest);
}

// include/pt_debug.h: the device time of one skin launch (the best of reps), into the pose's scratch copy
int pt_debug_skin_time(pt_pose* P, const float* xforms, size_t xformBytes, int which, int reps, float* msBest) {
    const bool live = poseLive(P);
    if (!live || !hasBones(P) || !msBest || reps < 1 || (which != PT_SKIN_PER_QUAD && which != PT_SKIN_PER_CORNER) || !xforms || P->nParts < 1 || xformBytes != (size_t)P->nParts * 96)
        return fail(PT_ERR_ARG, "pt_debug_skin_time: bad argument");
    if (P->rule == RULE_SKIN_DQ) return fail(PT_ERR_ARG, "pt_debug_skin_time: a DQ pose blends no matrices (pt_debug_skin_dq_time times its kernels)");
    return ruleTime(P, xforms, which, reps, "pt_debug_skin_time", msBest);
}

// include/pt_debug.h: the device time of the two launches of a DQ pose, records then corners (the best of reps), into the pose's scratch copy
int pt_debug_skin_dq_time(pt_pose* P, const float* xforms, size_t xformBytes, int reps, float* msBest) {
    const bool live = poseLive(P);
    if (!live || P->rule != RULE_SKIN_DQ || !msBest || reps < 1 || !xforms || P->nParts < 1 || xformBytes != (size_t)P->nParts * 96)
        return fail(PT_ERR_ARG, "pt_debug_skin_dq_time: bad argument");
    return ruleTime(P, xforms, 0, reps, "pt_debug_skin_dq_time", msBest);
}

// include/pt_debug.h: the pose's scratch copy as the last pt_pose_triangles / pt_debug_pose_time / pt_debug_skin_time / pt_debug_skin_dq_time left it
int pt_debug_pose_scratch(pt_pose* P, float* trisOut, size_t triBytes) {
    const bool live = poseLive(P);
    if (!live || !trisOut || !P->scratchReady || triBytes != (size_t)P->nTris * 160) return fail(PT_ERR_ARG, "pt_debug_pose_scratch: bad argument");
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipSetDevice(P->device));
    if (P->nTris) HIP_TRY(hipMemcpyAsync(trisOut, P->dScratch, triBytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PT_OK;
}

// ---- include/pt_morph.h

int pt_morph_attach(pt_pose* P, int nTargets, const int64_t* targetStart, size_t startBytes, const int32_t* entryCorner, size_t cornerBytes, const float* entryDelta,
                    size_t deltaBytes) {
    const bool live = poseLive(P);
    std::vector<unsigned char> moved;
    if (live && targetStart && entryCorner && entryDelta && !P->nTargets) { if (const int rc = movedCorners(P, moved)) return rc; }
    if (int rc = fail(ptp::checkMorphAttach(live, live && P->nTargets, nTargets, targetStart, startBytes, entryCorner, cornerBytes, entryDelta, deltaBytes,
                                            live ? (size_t)P->nTris : 0, moved.data())))
        return rc;
    if (P->stale) return fail(PT_ERR_SCENE, "pt_morph_attach: the scene was uploaded since pt_pose_create");
    ptp::MorphRows rows;
    ptp::morphRows(nTargets, targetStart, entryCorner, entryDelta, (size_t)P->nTris * 3, rows);
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipSetDevice(P->device));
    Dev<float> rest, w; Dev<int32_t> corner, row; Dev<ptp::MorphEntry> entry;       // the pose changes only once every allocation stands
    HIP_TRY(rest.reset(P->nTris ? (size_t)P->nTris * 160 : 16));
    if (P->nTris) HIP_TRY(hipMemcpyAsync(rest, P->dRest, (size_t)P->nTris * 160, hipMemcpyDeviceToDevice, st));
    HIP_TRY(corner.upload(rows.corners.data(), rows.corners.size() * 4, st));
    HIP_TRY(row.upload(rows.rowStart.data(), rows.rowStart.size() * 4, st));
    HIP_TRY(entry.upload(rows.entries.data(), rows.entries.size() * sizeof(ptp::MorphEntry), st));
    HIP_TRY(w.reset((size_t)nTargets * 4));
    HIP_TRY(hipStreamSynchronize(st));
    P->dMorphRest = std::move(rest); P->dMorphW = std::move(w); P->dMorphCorner = std::move(corner); P->dMorphRow = std::move(row); P->dMorphEntry = std::move(entry);
    P->nTargets = nTargets; P->nAffected = (int64_t)rows.corners.size();
    P->weights.assign((size_t)nTargets, 0.0f);
    return PT_OK;
}

int pt_morph_weights(pt_pose* P, const float* weights, size_t weightBytes) {
    const bool live = poseLive(P);
    if (int rc = fail(ptp::checkMorphWeights(live, live && P->nTargets, weights, weightBytes, live ? P->nTargets : 0))) return rc;
    P->weights.assign(weights, weights + P->nTargets);
    return PT_OK;
}

// include/pt_debug.h: the device time of one k_morph_corners launch (the best of reps) under the given weights, into the morphed rest pose
int pt_debug_morph_time(pt_pose* P, const float* weights, size_t weightBytes, int reps, float* msBest) {
    const bool live = poseLive(P);
    if (!msBest || reps < 1) return fail(PT_ERR_ARG, "pt_debug_morph_time: bad argument");
    if (ptp::checkMorphWeights(live, live && P->nTargets, weights, weightBytes, live ? P->nTargets : 0).code) return fail(PT_ERR_ARG, "pt_debug_morph_time: bad argument");
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipSetDevice(P->device));
    HIP_TRY(hipMemcpyAsync(P->dMorphW, weights, (size_t)P->nTargets * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return bestTime(st, reps, "pt_debug_morph_time", [&] {
        return ptMorphLaunch(P->dRest, P->dMorphCorner, P->dMorphRow, P->dMorphEntry, P->dMorphW, P->nAffected, P->dMorphRest, st) == hipSuccess;
    }, msBest);
}

// include/pt_debug.h: the kernel alone, under the weights last set (launched also when every weight is zero), and the morphed rest pose downloaded
int pt_debug_morph_rest(pt_pose* P, float* trisOut, size_t triBytes) {
    const bool live = poseLive(P);
    if (!live || !P->nTargets || !trisOut || triBytes != (size_t)P->nTris * 160) return fail(PT_ERR_ARG, "pt_debug_morph_rest: bad argument");
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipSetDevice(P->device));
    if (const int rc = morphRest(P, P->weights.data())) return rc;
    if (P->nTris) HIP_TRY(hipMemcpyAsync(trisOut, P->dMorphRest, triBytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PT_OK;
}

// ---- include/pt_normals.h

int pt_normals_attach(pt_pose* P, const int32_t* cornerVertex, size_t vertexBytes, int64_t nVertices, uint32_t flags) {
    const bool live = poseLive(P);
    std::vector<unsigned char> moved;
    if (live && cornerVertex && !P->hasNormals) { if (const int rc = movedCorners(P, moved)) return rc; }
    if (int rc = fail(ptp::checkNormalsAttach(live, live && P->hasNormals, cornerVertex, vertexBytes, nVertices, flags, live ? (size_t)P->nTris : 0, moved.data()))) return rc;
    if (P->stale) return fail(PT_ERR_SCENE, "pt_normals_attach: the scene was uploaded since pt_pose_create");
    ptp::NormalRows rows;
    ptp::normalRows(cornerVertex, (size_t)P->nTris, nVertices, rows);
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipSetDevice(P->device));
    Dev<int32_t> tri, row, corner, cornerRow; Dev<float> face;       // the pose changes only once every allocation stands
    HIP_TRY(tri.upload(rows.tris.data(), rows.tris.size() * 4, st));
    HIP_TRY(row.upload(rows.rowStart.data(), rows.rowStart.size() * 4, st));
    HIP_TRY(corner.upload(rows.corners.data(), rows.corners.size() * 4, st));
    HIP_TRY(cornerRow.upload(rows.cornerRow.data(), rows.cornerRow.size() * 4, st));
    HIP_TRY(face.reset(P->nTris ? (size_t)P->nTris * 16 : 16));
    HIP_TRY(hipStreamSynchronize(st));
    P->dNrmTri = std::move(tri); P->dNrmRow = std::move(row); P->dNrmCorner = std::move(corner); P->dNrmCornerRow = std::move(cornerRow); P->dNrmFace = std::move(face);
    P->nNrmTris = (int64_t)rows.tris.size(); P->nNrmRows = (int64_t)rows.verts.size(); P->nNrmCorners = (int64_t)rows.corners.size();
    P->normalsFlags = flags; P->hasNormals = true; P->normalsMode = 1;
    return PT_OK;
}

int pt_normals_mode(pt_pose* P, int on) {
    const bool live = poseLive(P);
    if (int rc = fail(ptp::checkNormalsMode(live, live && P->hasNormals, on))) return rc;
    P->normalsMode = on;
    return PT_OK;
}

// include/pt_debug.h: the pose under the weights last set and the rule's normals into the scratch copy once, then the device time of the faces
// launch plus the chosen statement of the gather over it (the best of reps)
int pt_debug_normals_time(pt_pose* P, const float* xforms, size_t xformBytes, int which, int reps, float* msBest) {
    const bool live = poseLive(P);
    if (!live || !P->hasNormals || !msBest || reps < 1 || (which != PT_NORMALS_PER_VERTEX && which != PT_NORMALS_PER_CORNER) || !xforms || P->nParts < 1 ||
        xformBytes != (size_t)P->nParts * 96)
        return fail(PT_ERR_ARG, "pt_debug_normals_time: bad argument");
    std::vector<float> tris((size_t)P->nTris * 40);
    if (const int rc = poseToHost(P, xforms, P->weights, 0, tris.data())) return rc;       // (the scratch copy holds the pose's rule's work afterwards; synchronised)
    // (a launch reads vertices and writes normals: every repetition gives the same bits)
    return bestTime(P->plan->stream, reps, "pt_debug_normals_time", [&] { return normalsInto(P, P->dScratch, (PtNormalsKernel)which) == 0; }, msBest);
}

// ---- include/pt_rig.h

namespace {

// steps 1-4 over the locals at dLocals (device) into `records`, level by level from the roots down; asynchronous on the plan's stream
int rigRun(pt_rig* G, const float* dLocals, float* records) {
    const hipStream_t st = G->pose->plan->stream;
    for (int l = 0; l < G->plan.levels(); l++) {
        const int first = G->plan.levelStart[(size_t)l], count = G->plan.levelStart[(size_t)l + 1] - first;
        HIP_TRY(ptRigLevelLaunch(G->dOrder, first, count, G->dParent, dLocals, G->hasBind ? (const float*)G->dBind : nullptr, G->dW, records, st));
    }
    return 0;
}

// include/pt_rig_mix.h step 1 for every layer, and where its keys lie: the table k_rig_mix takes by value.  The layers were checked
PtRigMixTable rigMixTable(pt_rig* G, const pt_rig_layer* layers, size_t layerBytes) {
    PtRigMixTable T = {};
    const size_t keyFloats = (size_t)G->n * PT_RIG_LOCAL_FLOATS;
    T.nLayers = (int32_t)(layerBytes / sizeof(pt_rig_layer));
    for (int l = 0; l < T.nLayers; l++) {
        const pt_rig_layer& y = layers[l];
        const ptp::RigMixStep s = ptp::rigMixStep(G->mixTimes[y.clip].data(), G->slots.nKeys[y.clip], y.wrap, y.t);
        const float* keys = G->dMixClip[y.clip];
        T.a[l] = keys + keyFloats * (size_t)s.ka; T.b[l] = keys + keyFloats * (size_t)s.kb; T.r[l] = keys;
        T.mask[l] = y.mask >= 0 ? (const float*)G->dMixMask[y.mask] : nullptr;
        T.u[l] = s.u; T.weight[l] = y.weight; T.mode[l] = y.mode;
    }
    return T;
}

// the mix of a table into dLocals; asynchronous on the plan's stream
int rigMixInto(pt_rig* G, const PtRigMixTable& mix) {
    HIP_TRY(hipSetDevice(G->pose->device));
    HIP_TRY(ptRigMixLaunch(mix, G->n, G->dLocals, G->pose->plan->stream));
    return 0;
}

// the records of a call into dR: of `locals` (host), with clip of the attached clip at time t (no NaN), or with mix of that table's layers;
// asynchronous on the plan's stream
int rigInto(pt_rig* G, bool clip, const float* locals, float t, const PtRigMixTable* mix = nullptr) {
    const hipStream_t st = G->pose->plan->stream;
    const size_t keyFloats = (size_t)G->n * PT_RIG_LOCAL_FLOATS;
    HIP_TRY(hipSetDevice(G->pose->device));
    if (G->n == 0) return 0;
    const float* src = G->dLocals;
    if (mix) { if (const int rc = rigMixInto(G, *mix)) return rc; }
    else if (!clip) HIP_TRY(hipMemcpyAsync(G->dLocals, locals, keyFloats * 4, hipMemcpyHostToDevice, st));
    else {
        int k; float u;
        const int exact = ptp::rigInterval(G->times.data(), G->nKeys, t, &k, &u);
        if (exact >= 0) src = G->dClip + keyFloats * (size_t)exact;                  // a key's own locals, bit for bit
        else HIP_TRY(ptRigBlendLaunch(G->dClip + keyFloats * (size_t)k, G->dClip + keyFloats * (size_t)(k + 1), u, G->n, G->dLocals, st));
    }
    return rigRun(G, src, G->dR);
}

// dR downloaded; the plan's stream is idle afterwards
int rigDownload(pt_rig* G, float* out) {
    const hipStream_t st = G->pose->plan->stream;
    if (G->n) HIP_TRY(hipMemcpyAsync(out, G->dR, (size_t)G->n * 96, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// the geometry calls after their argument checks: R on the device and, for the accepted state and the slow paths, on the host; then the pose's one path
int rigGeometry(pt_ctx* c, pt_rig* G, bool clip, const float* locals, float t, const float* ellip, size_t ellipBytes, double* rootCost, int* inPlace, const char* who,
                const PtRigMixTable* mix = nullptr) {
    pt_pose* P = G->pose;
    if (P->stale) return fail(PT_ERR_SCENE, std::string(who) + ": the scene was uploaded since pt_pose_create");
    std::vector<float> R((size_t)G->n * PT_POSE_RECORD_FLOATS);
    int rc;
    if ((rc = rigInto(G, clip, locals, t, mix)) || (rc = rigDownload(G, R.data()))) return rc;
    return poseGeometry(c, P, R.data(), R.size() * 4, G->n ? (const float*)G->dR : nullptr, ellip, ellipBytes, rootCost, inPlace, who);
}

}  // namespace

int pt_rig_create(pt_pose* P, const int32_t* parent, size_t parentBytes, const float* invBind, size_t bindBytes, pt_rig** out) {
    const bool live = poseLive(P);
    if (int rc = fail(ptp::checkRigCreate(P, live, parent, parentBytes, invBind, bindBytes, out, live ? P->nParts : 0))) return rc;
    pt_rig* G = new pt_rig();
    G->pose = P; G->n = P->nParts; G->hasBind = invBind != nullptr;
    ptp::rigPlan(parent, (size_t)G->n, G->plan);
    const hipStream_t st = P->plan->stream;
    const size_t n = (size_t)G->n;
    auto upload = [&]() {
        HIP_TRY(hipSetDevice(P->device));
        HIP_TRY(G->dOrder.upload(G->plan.order.data(), n * 4, st));
        HIP_TRY(G->dParent.upload(parent, n * 4, st));
        HIP_TRY(G->dBind.upload(invBind, invBind ? n * 48 : 0, st));
        HIP_TRY(G->dLocals.reset(std::max<size_t>(n * 48, 16)));
        HIP_TRY(G->dW.reset(std::max<size_t>(n * 48, 16)));
        HIP_TRY(G->dR.reset(std::max<size_t>(n * 96, 16)));
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
    if (const int rc = rigInto(G, false, locals, 0.0f)) return rc;
    return rigDownload(G, recordsOut);
}

int pt_rig_clip_attach(pt_rig* G, int nKeys, const float* times, size_t timeBytes, const float* values, size_t valueBytes) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigClipAttach(live, nKeys, times, timeBytes, values, valueBytes, live ? G->n : 0))) return rc;
    const hipStream_t st = G->pose->plan->stream;
    HIP_TRY(hipSetDevice(G->pose->device));
    Dev<float> clip;                                              // the rig changes only once the allocation stands
    HIP_TRY(clip.upload(values, valueBytes, st));
    HIP_TRY(hipStreamSynchronize(st));
    G->dClip = std::move(clip);
    G->times.assign(times, times + nKeys);
    G->nKeys = nKeys;
    return PT_OK;
}

int pt_rig_clip_records(pt_rig* G, float t, float* recordsOut, size_t recordBytes) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigClipRecords(live, live && G->nKeys > 0, t, recordsOut, recordBytes, live ? G->n : 0))) return rc;
    if (const int rc = rigInto(G, true, nullptr, t)) return rc;
    return rigDownload(G, recordsOut);
}

int pt_rig_pose_geometry(pt_ctx* c, pt_rig* G, const float* locals, size_t localBytes, const float* ellip, size_t ellipBytes, double* rootCost, int* inPlace) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigGeometry(false, c, live, live && G->pose->ctx == c, locals, localBytes, false, 0.0f, live ? G->n : 0, ellip, ellipBytes))) return rc;
    return rigGeometry(c, G, false, locals, 0.0f, ellip, ellipBytes, rootCost, inPlace, "pt_rig_pose_geometry");
}

int pt_rig_clip_pose_geometry(pt_ctx* c, pt_rig* G, float t, const float* ellip, size_t ellipBytes, double* rootCost, int* inPlace) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigGeometry(true, c, live, live && G->pose->ctx == c, nullptr, 0, live && G->nKeys > 0, t, live ? G->n : 0, ellip, ellipBytes))) return rc;
    return rigGeometry(c, G, true, nullptr, t, ellip, ellipBytes, rootCost, inPlace, "pt_rig_clip_pose_geometry");
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

// include/pt_debug.h: the device time of the rig's launches over the given locals, every level from the roots down (the best of reps), into dR
int pt_debug_rig_time(pt_rig* G, const float* locals, size_t localBytes, int reps, float* msBest) {
    const bool live = rigLive(G);
    if (!live || !msBest || reps < 1 || !locals || G->n < 1 || localBytes != (size_t)G->n * 48) return fail(PT_ERR_ARG, "pt_debug_rig_time: bad argument");
    const hipStream_t st = G->pose->plan->stream;
    HIP_TRY(hipSetDevice(G->pose->device));
    HIP_TRY(hipMemcpyAsync(G->dLocals, locals, localBytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    // (a launch reads locals and parents' W and writes W and R: every repetition gives the same bits)
    return bestTime(st, reps, "pt_debug_rig_time", [&] { return rigRun(G, G->dLocals, G->dR) == 0; }, msBest);
}

// ---- include/pt_rig_mix.h

int pt_rig_mix_clip(pt_rig* G, int slot, int nKeys, const float* times, size_t timeBytes, const float* values, size_t valueBytes) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigMixClip(live, slot, nKeys, times, timeBytes, values, valueBytes, live ? G->n : 0))) return rc;
    const hipStream_t st = G->pose->plan->stream;
    HIP_TRY(hipSetDevice(G->pose->device));
    Dev<float> clip;                                              // the rig changes only once the allocation stands
    HIP_TRY(clip.upload(values, valueBytes, st));
    HIP_TRY(hipStreamSynchronize(st));
    G->dMixClip[slot] = std::move(clip);
    G->mixTimes[slot].assign(times, times + nKeys);
    G->slots.nKeys[slot] = nKeys;
    return PT_OK;
}

int pt_rig_mix_mask(pt_rig* G, int slot, const float* weights, size_t weightBytes) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigMixMask(live, slot, weights, weightBytes, live ? G->n : 0))) return rc;
    const hipStream_t st = G->pose->plan->stream;
    HIP_TRY(hipSetDevice(G->pose->device));
    Dev<float> mask;
    HIP_TRY(mask.upload(weights, weightBytes, st));
    HIP_TRY(hipStreamSynchronize(st));
    G->dMixMask[slot] = std::move(mask);
    G->slots.mask[slot] = true;
    return PT_OK;
}

int pt_rig_mix_locals(pt_rig* G, const pt_rig_layer* layers, size_t layerBytes, float* localsOut, size_t localBytes) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigMixLayers(ptp::RIG_MIX_LOCALS, nullptr, live, true, live ? G->slots : ptp::RigMixSlots(), layers, layerBytes, localsOut, localBytes,
                                             live ? G->n : 0)))
        return rc;
    const hipStream_t st = G->pose->plan->stream;
    const PtRigMixTable T = rigMixTable(G, layers, layerBytes);
    if (const int rc = rigMixInto(G, T)) return rc;
    if (G->n) HIP_TRY(hipMemcpyAsync(localsOut, G->dLocals, localBytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PT_OK;
}

int pt_rig_mix_records(pt_rig* G, const pt_rig_layer* layers, size_t layerBytes, float* recordsOut, size_t recordBytes) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigMixLayers(ptp::RIG_MIX_RECORDS, nullptr, live, true, live ? G->slots : ptp::RigMixSlots(), layers, layerBytes, recordsOut, recordBytes,
                                             live ? G->n : 0)))
        return rc;
    const PtRigMixTable T = rigMixTable(G, layers, layerBytes);
    if (const int rc = rigInto(G, false, nullptr, 0.0f, &T)) return rc;
    return rigDownload(G, recordsOut);
}

int pt_rig_mix_pose_geometry(pt_ctx* c, pt_rig* G, const pt_rig_layer* layers, size_t layerBytes, const float* ellip, size_t ellipBytes, double* rootCost, int* inPlace) {
    const bool live = rigLive(G);
    if (int rc = fail(ptp::checkRigMixLayers(ptp::RIG_MIX_GEOMETRY, c, live, live && G->pose->ctx == c, live ? G->slots : ptp::RigMixSlots(), layers, layerBytes, ellip,
                                             ellipBytes, live ? G->n : 0)))
        return rc;
    const PtRigMixTable T = rigMixTable(G, layers, layerBytes);
    return rigGeometry(c, G, false, nullptr, 0.0f, ellip, ellipBytes, rootCost, inPlace, "pt_rig_mix_pose_geometry", &T);
}

// include/pt_debug.h: the device time of the mix's one launch over the given layers (the best of reps), into dLocals
int pt_debug_rig_mix_time(pt_rig* G, const pt_rig_layer* layers, size_t layerBytes, int reps, float* msBest) {
    const bool live = rigLive(G);
    if (!live || !msBest || reps < 1 || G->n < 1) return fail(PT_ERR_ARG, "pt_debug_rig_mix_time: bad argument");
    if (ptp::checkRigMixLayers(ptp::RIG_MIX_LOCALS, nullptr, true, true, G->slots, layers, layerBytes, msBest, (size_t)G->n * 48, G->n).code)      // (the layers' checks; no output here)
        return fail(PT_ERR_ARG, "pt_debug_rig_mix_time: bad argument");
    const hipStream_t st = G->pose->plan->stream;
    HIP_TRY(hipSetDevice(G->pose->device));
    const PtRigMixTable T = rigMixTable(G, layers, layerBytes);
    // (a launch reads keys and masks and writes dLocals: every repetition gives the same bits)
    return bestTime(st, reps, "pt_debug_rig_mix_time", [&] { return rigMixInto(G, T) == 0; }, msBest);
}
