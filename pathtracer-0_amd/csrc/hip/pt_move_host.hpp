// pt_move_host.hpp — the host half of pt_move_geometry (include/pt_move.h) and of pt_debug_scene_records (include/pt_debug.h), behind the C ABI
// (included at the end of pt_image.hpp, inside pt_hip.hip's extern "C" block, where pt_ctx and its helpers are in scope; not a translation unit).
// The kernels are pt_move.hip's, behind pt_move_launch.hpp; the refit is pt_refit.hip's, whose plan (pt_refit_state.hpp) holds the new binding 3 and
// the refit binding 10 on the device; what a patch rewrites, and the map it needs, is pt_scene_move.hpp's.
//
// The roots, the group boxes and the ellipsoid records — at most a few thousand small records — are computed on the HOST, from the binding 10 the call
// downloads anyway for the context's host copy, through the functions layoutScene itself calls, and uploaded into the arrays that exist.
//
// What keys the plan's map: the topology digest is compared on EVERY call (its cost is part of the call times of DESIGN.md 2.21), not cached per upload generation —
// the context counts scene uploads as one number, and a cache keyed by a context's address could outlive it; so the map is right for any context
// whose digest matches, and it is remade only when bfs_nodes differs.  The stride, the group shift and the cull switch are read from the context
// at each call.
extern "C++" {
#include "pt_refit_state.hpp"
#include "pt_move_launch.hpp"
}
#include "../../../include/pt_move.h"

namespace {

const char* const MOVE_UNORDERED = "a node box with min > max or a NaN";      // layoutScene's reason (pt_scene_layout.hpp, modes())
const char* const MOVE_TRIMAT = "triangle material index out of range (SURVEY.md Q-14: OBJ faces before any o/g line get -1)";

uint64_t moveDigest(const SceneBuffers& b) {
    return ptr::topologyDigest(b.bvhtree.data(), b.bvhtree.size(), b.leaftris.data(), b.leaftris.size(), b.objidx.data(), b.objidx.size(), b.bvhdata.data(),
                               b.bvhdata.size());
}
int moveForeignPlan() { return fail(PT_ERR_SCENE, "pt_move_geometry: the plan was not made from this context's scene (bindings 11, 12, 13 or the leaf ranges of binding 10 differ)"); }

// what pt_set_buffer records for the accepted uploads of 3, 10 and, when given, 7
void moveAccepted(pt_ctx* c, bool ellip) {
    c->hist.uploadBegins();
    c->hist.sceneBufferAccepted(PT_BIND_TRIANGLES);
    c->hist.sceneBufferAccepted(PT_BIND_BVHDATA);
    if (ellip) c->hist.sceneBufferAccepted(PT_BIND_ELLIPSOIDS);
}

// the slow path of a single context: the new buffers become the host copies and the scene is built; a scene that does not build leaves them as they were
int moveRebuild(pt_ctx* c, SceneBuffers& host, std::vector<float>& data, const float* tris, size_t triBytes, const float* ellip, size_t ellipBytes) {
    std::vector<float> newTris(tris, tris + triBytes / 4), newEllip;
    if (ellip) newEllip.assign(ellip, ellip + ellipBytes / 4);
    host.tris.swap(newTris); host.bvhdata.swap(data);
    if (ellip) c->buf.ellip.swap(newEllip);
    const int rc = buildScene(c);
    if (rc) {
        host.tris.swap(newTris); host.bvhdata.swap(data);
        if (ellip) c->buf.ellip.swap(newEllip);
        return rc;
    }
    moveAccepted(c, ellip != nullptr);
    return 0;
}

// a multi-stream / multi-GPU context: the sequence of include/pt_move.h through the public calls, then every replica builds
int moveMulti(pt_ctx* c, pt_refit_plan* P, const float* tris, size_t triBytes, const float* ellip, size_t ellipBytes, double* rootCost) {
    if (!c->multi->staleBindings.empty()) return fail(PT_ERR_SCENE, MULTI_UPLOAD_FAILED);
    SceneBuffers* host = nullptr;                                 // the first stream's copies (a group's streams are never behind a pose)
    if (const int rc = settledScene(c->multi->kids[0], &host)) return rc;
    if (moveDigest(*host) != P->digest || host->bvhdata.size() * 4 != P->dataBytes) return moveForeignPlan();
    std::vector<float> data(std::max<size_t>(P->dataBytes / 4, 1));
    std::vector<double> cost(std::max(P->s.nRoots, 1));
    int rc;
    if ((rc = pt_refit_run(P, tris, triBytes, data.data(), cost.data()))) return rc;
    if ((rc = pt_set_buffer(c, PT_BIND_TRIANGLES, tris, triBytes)) || (rc = pt_set_buffer(c, PT_BIND_BVHDATA, data.data(), P->dataBytes))) return rc;
    if (ellip && (rc = pt_set_buffer(c, PT_BIND_ELLIPSOIDS, ellip, ellipBytes))) return rc;
    if ((rc = multiFlushAndBuild(*c->multi))) return rc;
    if (rootCost) std::copy(cost.begin(), cost.begin() + P->s.nRoots, rootCost);
    return PT_OK;
}

// THE PATCH on the device: from here on the context's records change.  P's dTris / dData hold the new binding 3 and the refit binding 10, its stream
// is idle; the kernels run on the context's.  roots: the context's root records with the new boxes (moveRoots).  Synchronous; *unordered: a node box
// the patch wrote has min > max or a NaN.
int movePatchRecords(pt_ctx* c, pt_refit_plan* P, const std::vector<ObjRoot>& roots, const float* ellip, int* unordered) {
    const hipStream_t s = c->stream;
    PtMovePatch p{};
    p.tris = P->dTris; p.data = P->dData; p.child = P->dMapChild; p.triRecs = c->dTris; p.nTriRecs = c->sc.nTriRecs; p.shade = c->dShade; p.nTris = c->sc.nTris;
    p.nodes = c->dNodes; p.nodes80 = c->dNodes80; p.nInner = c->sc.nNodes; p.stride = c->built.asmNodeStride; p.flag = P->dFlag;
    HIP_TRY(ptMovePatchLaunch(p, s));
    HIP_TRY(hipMemcpyAsync(c->dRoots, roots.data(), roots.size() * sizeof(ObjRoot), hipMemcpyHostToDevice, s));
    std::vector<EllipRec> recs;
    if (ellip) {
        recs.resize(c->dEllip.bytes / sizeof(EllipRec));
        std::memset(recs.data(), 0, recs.size() * sizeof(EllipRec));
        ptl::moveEllipsoids(ellip, recs);
        HIP_TRY(hipMemcpyAsync(c->dEllip, recs.data(), recs.size() * sizeof(EllipRec), hipMemcpyHostToDevice, s));
    }
    *unordered = 0;
    HIP_TRY(hipMemcpyAsync(unordered, P->dFlag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// the tail of an in-place commit, of a move and of a pose (pt_pose_host.hpp) alike: movePatchRecords has succeeded and the caller has recorded its own
// side (a move: the host copies of bindings 3 and 10; a pose: c->behind and its accepted state).  The ellipsoids' host copy, what pt_set_buffer
// records, and — the modes assume ordered boxes — the scene build when the patch wrote an unordered box on an eligible 80-byte stride: the build
// decides (and settles).  *rebuilt: it did
int moveCommitted(pt_ctx* c, const float* ellip, size_t ellipBytes, int unordered, bool* rebuilt) {
    if (ellip) c->buf.ellip.assign(ellip, ellip + ellipBytes / 4);
    moveAccepted(c, ellip != nullptr);
    *rebuilt = false;
    if (unordered && c->built.asmEligible && c->built.asmNodeStride == 80) {
        if (const int rc = buildScene(c)) { c->sceneDirty = true; return rc; }
        *rebuilt = true;
    }
    return 0;
}

// the map of the record order, made by the first call and kept while bfs_nodes holds (reads the host copies, settled)
int moveEnsureMap(pt_ctx* c, pt_refit_plan* P) {
    if (P->mapValid && P->mapBfsNodes == c->opt.bfsNodes) return 0;
    std::string err;
    SceneBuffers* host = nullptr;
    if (const int rc = settledScene(c, &host)) return rc;
    P->mapValid = false;
    if (const int rc = ptl::moveMapOrder(*host, c->opt, P->map, err)) return fail(rc, err);
    HIP_TRY(P->dMapChild.upload(P->map.child.data(), P->map.child.size() * 4, P->stream));
    HIP_TRY(hipStreamSynchronize(P->stream));
    P->mapBfsNodes = c->opt.bfsNodes; P->mapValid = true;
    return 0;
}
// whether the map is of what was built (it is while the digest holds; the scene build decides otherwise)
bool moveMapFits(const pt_ctx* c, const pt_refit_plan* P) {
    const ptl::MoveMap& map = P->map;
    return map.nInner == c->sc.nNodes && map.numObj == c->sc.numObj &&
           c->dRoots.bytes / sizeof(ObjRoot) == (size_t)std::max(map.numObj, 8) + (map.numObj > 8 ? 64 : 0) && (size_t)map.nRows * 32 == P->dataBytes;
}

// pt_move_geometry itself; the entry point below adds what the call means for the context's poses (include/pt_pose.h), whose slow paths come here
int moveGeometry(pt_ctx* c, pt_refit_plan* P, const float* tris, size_t triBytes, const float* ellip, size_t ellipBytes, double* rootCost, int* inPlace) {
    if (!c) return fail(PT_ERR_ARG, "pt_move_geometry: null context");
    if (!pt_refit_live_(P)) return fail(PT_ERR_ARG, "pt_move_geometry: null or destroyed plan");
    if (!tris) return fail(PT_ERR_ARG, "pt_move_geometry: null tris");
    if (triBytes != (size_t)P->nTris * 160) return fail(PT_ERR_ARG, "pt_move_geometry: tri_bytes != n_tris * 160");
    if (ellip && ellipBytes % 4) return fail(PT_ERR_ARG, "pt_move_geometry: ellip_bytes must be a multiple of 4 bytes");
    if (P->device != firstStream(c)->device) return fail(PT_ERR_ARG, "pt_move_geometry: the plan lives on another device than the context");
    if (c->multi) {
        const int rc = moveMulti(c, P, tris, triBytes, ellip, ellipBytes, rootCost);
        if (!rc && inPlace) *inPlace = 0;
        return rc;
    }
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = flushStream(c))) return rc;                         // submitted frames are rendered in the old scene
    SceneBuffers* host = nullptr;                                 // the host copies are read below, and the plan may be the pose's they are behind on
    if ((rc = settledScene(c, &host))) return rc;
    if (c->sceneDirty && (rc = buildScene(c))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (moveDigest(*host) != P->digest || host->bvhdata.size() * 4 != P->dataBytes) return moveForeignPlan();
    if (ellip) { std::string err; if ((rc = ptl::ellipsoidsUsable(ellip, ellipBytes / 4, c->sc.numMat, err))) return fail(rc, err); }
    bool rebuild = c->asmWhyNot == MOVE_UNORDERED || (ellip && !ptl::ellipPatchable(c->buf.ellip, ellip, ellipBytes / 4)) || host->tris.size() / 40 != (size_t)P->nTris;

    // the refit: the plan's working copy only.  Then the material check, where the records' ids are the plan's triangles'
    if ((rc = pt_refit_device_(P, tris, triBytes, "pt_move_geometry"))) return rc;
    const hipStream_t ps = P->stream;
    if (!rebuild) {
        int flag = 0;
        HIP_TRY(ptMoveCheckLaunch(c->dTris, c->sc.nTriRecs, P->dTris, c->sc.numMat, P->dFlag, ps));
        HIP_TRY(hipMemcpyAsync(&flag, P->dFlag, 4, hipMemcpyDeviceToHost, ps));
        HIP_TRY(hipStreamSynchronize(ps));
        if (flag) return fail(PT_ERR_SCENE, MOVE_TRIMAT);
    }
    if (!rebuild && (rc = moveEnsureMap(c, P))) return rc;
    ptl::MoveMap& map = P->map;
    std::vector<ObjRoot> roots(c->dRoots.bytes / sizeof(ObjRoot));
    if (!rebuild && !moveMapFits(c, P)) rebuild = true;           // (not what was built: cannot happen while the digest holds; the scene build decides)

    std::vector<float> data(P->dataBytes / 4);
    std::vector<double> cost(std::max(P->s.nRoots, 1));
    if (P->dataBytes) HIP_TRY(hipMemcpyAsync(data.data(), P->dData, P->dataBytes, hipMemcpyDeviceToHost, ps));
    if (P->s.nRoots > 0) HIP_TRY(hipMemcpyAsync(cost.data(), P->dRootCost, (size_t)P->s.nRoots * 8, hipMemcpyDeviceToHost, ps));
    if (!rebuild) HIP_TRY(hipMemcpyAsync(roots.data(), c->dRoots, roots.size() * sizeof(ObjRoot), hipMemcpyDeviceToHost, ps));
    HIP_TRY(hipStreamSynchronize(ps));

    if (!rebuild) {
        // ---- the patch: from here on the context's records change
        map.asmStride = c->built.asmNodeStride; map.asmGroupShift = c->asmGroupShift; map.asmNoRootCull = c->opt.asmNoRootCull;
        ptl::moveRoots(map, data.data(), roots.data());
        int unordered = 0;
        if ((rc = movePatchRecords(c, P, roots, ellip, &unordered))) return rc;
        host->tris.assign(tris, tris + triBytes / 4);
        host->bvhdata.swap(data);
        if ((rc = moveCommitted(c, ellip, ellipBytes, unordered, &rebuild))) return rc;
    } else if ((rc = moveRebuild(c, *host, data, tris, triBytes, ellip, ellipBytes))) {
        return rc;
    }
    if (rootCost) std::copy(cost.begin(), cost.begin() + P->s.nRoots, rootCost);
    if (inPlace) *inPlace = rebuild ? 0 : 1;
    return PT_OK;
}

}  // namespace

int pt_move_geometry(pt_ctx* c, pt_refit_plan* P, const float* tris, size_t triBytes, const float* ellip, size_t ellipBytes, double* rootCost, int* inPlace) {
    const int rc = moveGeometry(c, P, tris, triBytes, ellip, ellipBytes, rootCost, inPlace);
    if (!rc) posesStale(c);                                       // binding 3 is no longer what a pose's rest pose would give
    return rc;
}

// One device record array of the built scene read back (tests): which = 0 nodes, 1 nodes80, 2 tris, 3 shade, 4 roots, 5 ellip, 6 triObj
int pt_debug_scene_records(pt_ctx* c, int which, void* out, size_t cap, size_t* bytes) {
    if (!c || !bytes) return fail(PT_ERR_ARG, "pt_debug_scene_records: null argument");
    if (c->multi) return fail(PT_ERR_ARG, "pt_debug_scene_records: a multi-stream context holds one scene per stream");
    if (c->sceneDirty) return fail(PT_ERR_ARG, "pt_debug_scene_records: the scene is not built (an upload or option since the last render)");
    const void* src = nullptr; size_t n = 0;
    const size_t nTris = (size_t)std::max(c->sc.nTris, 1);
    switch (which) {
        case 0: src = c->dNodes; n = (size_t)c->sc.nNodes * 64; break;
        case 1: src = c->dNodes80; n = c->dNodes80.bytes; break;
        case 2: src = c->dTris; n = (size_t)c->sc.nTriRecs * 48; break;
        case 3: src = c->dShade; n = nTris * 64; break;
        case 4: src = c->dRoots; n = c->dRoots.bytes; break;
        case 5: src = c->dEllip; n = c->dEllip.bytes; break;
        case 6: src = c->dTriObj; n = nTris * 4; break;
        default: return fail(PT_ERR_ARG, "pt_debug_scene_records: which must be 0 (nodes), 1 (nodes80), 2 (tris), 3 (shade), 4 (roots), 5 (ellip) or 6 (triObj)");
    }
    *bytes = n;
    if (cap == 0) return PT_OK;
    if (!out || cap < n) return fail(PT_ERR_ARG, "pt_debug_scene_records: the buffer is smaller than the array");
    HIP_TRY(hipSetDevice(c->device));
    if (const int rc = flushStream(c)) return rc;
    if (n) {
        HIP_TRY(hipMemcpyAsync(out, src, n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return PT_OK;
}
