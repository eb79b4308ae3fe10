// pt_pose_host.hpp — the pose object behind the C ABI and everything that belongs to one pose: the entry points of include/pt_pose.h, pt_skin.h,
// pt_skin_dq.h, pt_morph.h and pt_normals.h, and what pt_context.hpp declares (settleScene and its kin).  Included at the end of pt_image.hpp after
// pt_move_host.hpp, inside pt_hip.hip's extern "C" block, where pt_ctx, the in-place move and their helpers are in scope; not a translation unit.
//
// It takes: the kernels behind the five *_launch.hpp headers included below; the argument checks, inverted indices and CPU statements of the five
// *_rule.hpp headers; the refit's second half (pt_refit_kernels_) and the patch of the context's records (movePatchRecords, moveCommitted) from
// pt_move_host.hpp.  Of the rig (pt_rig_host.hpp, included after this file) it needs rigsFree alone; the timers and readers of include/pt_debug.h
// for this family are pt_geom_debug_host.hpp's.
//
// What a reader must know.  One object, three rules (PoseRule), told apart in ruleLaunch and nowhere else; a morph ahead of the rule and normals
// behind it belong to a pose of any rule, and poseInto runs the chain.  Every call ends with the plan's stream idle.  plan->dTris: static
// triangles (part -1) are the rest pose's from creation on and are never written again by a kernel (the slow path's upload writes the same
// values); the others hold the pose last run.  While the context is behind on this pose (c->behind == pose), dTris and dData are the bindings 3
// and 10 a settle delivers: a refused pose is undone by running the last accepted one (PoseState) again.
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
#include <set>
}
#include "../../../include/pt_pose.h"
#include "../../../include/pt_skin.h"
#include "../../../include/pt_skin_dq.h"
#include "../../../include/pt_morph.h"
#include "../../../include/pt_normals.h"

struct pt_rig;                          // include/pt_rig.h, pt_rig_host.hpp

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
    Dev<float> dDq;                     // RULE_SKIN_DQ: the dual quaternions of the records
    bool scratchReady = false;          // dScratch holds the rest pose's static triangles (pt_pose_triangles, the slow paths)
    int rowsFor = -1, nRows = 0;        // dRowIds lists the rows of the plan's map made under this bfs_nodes
    PoseState accepted;                 // the last accepted pose: a refused call is undone by running it again
    // include/pt_morph.h: nTargets > 0 once a morph is attached.  dMorphRest is a second copy of the rest pose, of which the kernel rewrites the
    // affected corners (all of them, on every morphed call) and nothing else
    int nTargets = 0; int64_t nAffected = 0;
    Dev<float> dMorphRest, dMorphW; Dev<int32_t> dMorphCorner, dMorphRow; Dev<ptp::MorphEntry> dMorphEntry;
    std::vector<float> weights;         // as pt_morph_weights set them last (after the attach: zeros)
    // include/pt_normals.h: hasNormals once normals are attached.  The inverted index of pt_normals_rule.hpp (the listed triangles, the row starts
    // of the non-empty vertices, their corners, per corner its row) and the face vectors, indexed by triangle id
    bool hasNormals = false; uint32_t normalsFlags = 0;
    int64_t nNrmTris = 0, nNrmRows = 0, nNrmCorners = 0;
    Dev<int32_t> dNrmTri, dNrmRow, dNrmCorner, dNrmCornerRow; Dev<float> dNrmFace;
    int normalsMode = 0;                // as pt_normals_mode set it last (after the attach: 1)
    bool stale = false;                 // pt_set_buffer ran after the create: staleRefused
    std::vector<pt_rig*> rigs;          // include/pt_rig.h: the rigs attached to this pose, which go with it
};

namespace {

// sizes, each named once
constexpr size_t TRI_FLOATS = 40, TRI_BYTES = TRI_FLOATS * 4;              // a triangle record of binding 3
constexpr size_t RECORD_BYTES = PT_POSE_RECORD_FLOATS * 4;                 // a pose record
constexpr size_t SKIN_WORDS = 3 * PT_SKIN_SLOTS;                           // the slots of a triangle's three corners, in dBone and in dWeight
constexpr size_t DQ_BYTES = 32;                                            // a record's dual quaternion
constexpr size_t FACE_BYTES = 16;                                          // a triangle's face vector
constexpr size_t ROW_FLOATS = 8;                                           // a row of binding 10 as k_pose_gather collects it
constexpr size_t MOTION_BYTES = 3 * sizeof(float4);                        // a triangle's record of poseMotionRecords
size_t atLeast16(size_t bytes) { return std::max<size_t>(bytes, 16); }     // an allocation of no bytes is one of 16: every pointer handed to a kernel is one

std::mutex g_posesMutex;                // over the live poses and (pt_rig_host.hpp) the live rigs
std::set<pt_pose*> g_poses;             // the live poses: a destroyed one is refused, not followed
constexpr PtPoseKernel POSE_KERNEL = PT_POSE_PER_QUAD;      // the faster of the two at 100 k and at 1 M triangles (scripts/pose_probe.py); pt_debug_pose_time runs either
constexpr PtNormalsKernel NORMALS_KERNEL = PT_NORMALS_PER_CORNER;   // 5 % slower on C4's mesh, 10 % faster on the 1 M height field: the shorter summed over both (71.9 against 77.4 us), and twice as fast on a table with one long row (scripts/normals_probe.py); pt_debug_normals_time runs either
constexpr PtSkinKernel SKIN_KERNEL = PT_SKIN_PER_CORNER;    // faster with four slots at 100 k and at 1 M triangles, tied at 100 k and 2 % slower at 1 M with two: the shorter summed over both slot counts at 1 M (scripts/skin_probe.py); pt_debug_skin_time runs either
constexpr int RULE_KERNEL[3] = {POSE_KERNEL, SKIN_KERNEL, 0};    // by PoseRule: the statement poseInto runs (the DQ rule has one)

bool poseLive(pt_pose* p) {
    std::lock_guard<std::mutex> g(g_posesMutex);
    return p && g_poses.count(p);
}

// THE refusal of a pose whose scene was uploaded again, under the name of the call that meets it
int staleRefused(const char* who) { return fail(PT_ERR_SCENE, std::string(who) + ": the scene was uploaded since pt_pose_create"); }

void rigsFree(pt_pose* P);              // pt_rig_host.hpp: the pose's rigs leave the registry and are deleted

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

// the whole rest pose into dst; asynchronous on the plan's stream
int restInto(pt_pose* P, float* dst) {
    if (P->nTris) HIP_TRY(hipMemcpyAsync(dst, P->dRest, (size_t)P->nTris * TRI_BYTES, hipMemcpyDeviceToDevice, P->plan->stream));
    return 0;
}

// the pose of `xforms` (host; nullptr: the rest pose, unmorphed, its normals as they are) under the morph weights `weights` (host; empty: no morph,
// or every weight 0) and the normals mode `mode` (1: recomputed where normals are attached) into dst, which holds the rest pose's static
// triangles; asynchronous on the plan's stream.  onDevice: where the same records lie on the device already (a rig's dR): copied from there,
// not uploaded
int poseInto(pt_pose* P, const float* xforms, const std::vector<float>& weights, int mode, float* dst, const float* onDevice = nullptr) {
    const hipStream_t st = P->plan->stream;
    if (!xforms || P->nParts == 0) return restInto(P, dst);      // (n_parts == 0: a morph has no entries)
    // every weight +-0: the morphed rest pose is the rest pose, bit for bit (the header's consequence 1), and the launch is skipped
    bool morphed = false;
    for (const float w : weights) morphed = morphed || w != 0.0f;
    if (morphed) { if (const int rc = morphRest(P, weights.data())) return rc; }
    const float* rest = morphed ? (const float*)P->dMorphRest : (const float*)P->dRest;
    const size_t bytes = (size_t)P->nParts * RECORD_BYTES;
    HIP_TRY(P->dX.ensure(bytes));
    if (onDevice) HIP_TRY(hipMemcpyAsync(P->dX, onDevice, bytes, hipMemcpyDeviceToDevice, st));
    else HIP_TRY(hipMemcpyAsync(P->dX, xforms, bytes, hipMemcpyHostToDevice, st));
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

// the scratch copy exists and holds the rest pose's static triangles: made, and the rest pose copied in, by the first call; asynchronous on the
// plan's stream
int scratchStands(pt_pose* P) {
    if (P->scratchReady) return 0;
    HIP_TRY(P->dScratch.reset(atLeast16((size_t)P->nTris * TRI_BYTES)));
    if (const int rc = restInto(P, P->dScratch)) return rc;
    P->scratchReady = true;
    return 0;
}

// P = the rule applied to the rest pose, on the host; the plan's working copies are not touched
int poseToHost(pt_pose* P, const float* xforms, const std::vector<float>& weights, int mode, float* out) {
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipSetDevice(P->device));
    int rc;
    if ((rc = scratchStands(P)) || (rc = poseInto(P, xforms, weights, mode, P->dScratch))) return rc;
    if (P->nTris) HIP_TRY(hipMemcpyAsync(out, P->dScratch, (size_t)P->nTris * TRI_BYTES, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// which corners the pose's rule moves, a byte per corner: from the part ids or the bone table, which lie on the device (no triangles: left empty)
int movedCorners(pt_pose* P, std::vector<unsigned char>& moved) {
    if (!P->nTris) return 0;
    const hipStream_t st = P->plan->stream;
    const bool bones = hasBones(P);
    HIP_TRY(hipSetDevice(P->device));
    moved.resize((size_t)P->nTris * 3);
    std::vector<int32_t> words((size_t)P->nTris * (bones ? SKIN_WORDS : 1));
    HIP_TRY(hipMemcpyAsync(words.data(), bones ? P->dBone : P->dPart, words.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t q = 0; q < moved.size(); q++) moved[q] = (bones ? words[PT_SKIN_SLOTS * q] : words[q / 3]) >= 0;
    return 0;
}

void poseFree(pt_pose* P) {
    hipSetDevice(P->device);
    rigsFree(P);
    pt_refit_destroy(P->plan);
    delete P;
}

// ---- what pt_context.hpp declares

int settleScene(pt_ctx* c) {
    pt_pose* P = c->behind;
    if (!P) return 0;
    pt_refit_plan* plan = P->plan;
    HIP_TRY(hipSetDevice(c->device));
    c->buf.tris.resize((size_t)P->nTris * TRI_FLOATS);
    c->buf.bvhdata.resize(plan->dataBytes / 4);
    if (P->nTris) HIP_TRY(hipMemcpyAsync(c->buf.tris.data(), plan->dTris, (size_t)P->nTris * TRI_BYTES, hipMemcpyDeviceToHost, plan->stream));
    if (plan->dataBytes) HIP_TRY(hipMemcpyAsync(c->buf.bvhdata.data(), plan->dData, plan->dataBytes, hipMemcpyDeviceToHost, plan->stream));
    HIP_TRY(hipStreamSynchronize(plan->stream));
    c->behind = nullptr;
    return 0;
}

int poseMotionRecords(pt_ctx* on, const float4* then, int nThen, Dev<float4>& out, int* nTri) {
    const pt_pose* P = on->behind;                                // (its plan's stream is idle: every pose call ends synchronised)
    const int n = (int)P->nTris;
    HIP_TRY(hipSetDevice(on->device));
    HIP_TRY(out.ensure(atLeast16((size_t)n * MOTION_BYTES)));     // (kept from call to call: the count cannot change while the context is behind)
    if (n == 0) HIP_TRY(hipMemsetAsync(out, 0, sizeof(float4), on->stream));     // (motionPack's one zero record)
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
    std::vector<float> tris((size_t)P->nTris * TRI_FLOATS);
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
        HIP_TRY(P->dRest.upload(b.tris.data(), nTris * TRI_BYTES, st));
        if (hasBones(P)) {
            HIP_TRY(P->dBone.upload(bone, nTris * SKIN_WORDS * 4, st));
            HIP_TRY(P->dWeight.upload(weight, nTris * SKIN_WORDS * 4, st));
        } else HIP_TRY(P->dPart.upload(triPart, nTris * 4, st));
        HIP_TRY(P->dX.reset(atLeast16((size_t)nParts * RECORD_BYTES)));
        if (rule == RULE_SKIN_DQ) HIP_TRY(P->dDq.reset(atLeast16((size_t)nParts * DQ_BYTES)));
        if ((rc = restInto(P, plan->dTris))) return rc;           // the static triangles, once
        HIP_TRY(hipStreamSynchronize(st));
        return 0;
    };
    if ((rc = upload())) { const std::string msg = g_err; poseFree(P); return fail(rc, msg); }
    { std::lock_guard<std::mutex> g(g_posesMutex); g_poses.insert(P); }
    c->poses.push_back(P);
    *out = P;
    return PT_OK;
}

// pt_pose_geometry after its argument checks, under the name `who` of the call it serves; onDevice: as for poseInto
int poseGeometry(pt_ctx* c, pt_pose* P, const float* xforms, size_t xformBytes, const float* onDevice, const float* ellip, size_t ellipBytes, double* rootCost, int* inPlace,
                 const char* who) {
    if (P->stale) return staleRefused(who);
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
        HIP_TRY(P->dRows.reset(atLeast16(ids.size() * ROW_FLOATS * 4)));
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
    std::vector<float> rows((size_t)P->nRows * ROW_FLOATS);
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

// ---- include/pt_pose.h, pt_skin.h, pt_skin_dq.h

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

// ---- include/pt_morph.h

int pt_morph_attach(pt_pose* P, int nTargets, const int64_t* targetStart, size_t startBytes, const int32_t* entryCorner, size_t cornerBytes, const float* entryDelta,
                    size_t deltaBytes) {
    const bool live = poseLive(P);
    std::vector<unsigned char> moved;
    if (live && targetStart && entryCorner && entryDelta && !P->nTargets) { if (const int rc = movedCorners(P, moved)) return rc; }
    if (int rc = fail(ptp::checkMorphAttach(live, live && P->nTargets, nTargets, targetStart, startBytes, entryCorner, cornerBytes, entryDelta, deltaBytes,
                                            live ? (size_t)P->nTris : 0, moved.data())))
        return rc;
    if (P->stale) return staleRefused("pt_morph_attach");
    ptp::MorphRows rows;
    ptp::morphRows(nTargets, targetStart, entryCorner, entryDelta, (size_t)P->nTris * 3, rows);
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipSetDevice(P->device));
    Dev<float> rest, w; Dev<int32_t> corner, row; Dev<ptp::MorphEntry> entry;       // the pose changes only once every allocation stands
    HIP_TRY(rest.reset(atLeast16((size_t)P->nTris * TRI_BYTES)));
    if (const int rc = restInto(P, rest)) return rc;
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

// ---- include/pt_normals.h

int pt_normals_attach(pt_pose* P, const int32_t* cornerVertex, size_t vertexBytes, int64_t nVertices, uint32_t flags) {
    const bool live = poseLive(P);
    std::vector<unsigned char> moved;
    if (live && cornerVertex && !P->hasNormals) { if (const int rc = movedCorners(P, moved)) return rc; }
    if (int rc = fail(ptp::checkNormalsAttach(live, live && P->hasNormals, cornerVertex, vertexBytes, nVertices, flags, live ? (size_t)P->nTris : 0, moved.data()))) return rc;
    if (P->stale) return staleRefused("pt_normals_attach");
    ptp::NormalRows rows;
    ptp::normalRows(cornerVertex, (size_t)P->nTris, nVertices, rows);
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipSetDevice(P->device));
    Dev<int32_t> tri, row, corner, cornerRow; Dev<float> face;       // the pose changes only once every allocation stands
    HIP_TRY(tri.upload(rows.tris.data(), rows.tris.size() * 4, st));
    HIP_TRY(row.upload(rows.rowStart.data(), rows.rowStart.size() * 4, st));
    HIP_TRY(corner.upload(rows.corners.data(), rows.corners.size() * 4, st));
    HIP_TRY(cornerRow.upload(rows.cornerRow.data(), rows.cornerRow.size() * 4, st));
    HIP_TRY(face.reset(atLeast16((size_t)P->nTris * FACE_BYTES)));
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
