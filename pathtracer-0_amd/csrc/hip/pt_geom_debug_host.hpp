// pt_geom_debug_host.hpp — the pose family's host half of include/pt_debug.h: the eight timers (pt_debug_pose_time, _skin_time, _skin_dq_time,
// _morph_time, _normals_time, _rig_time, _rig_mix_time, _rig_ik_time) and the two readers (pt_debug_pose_scratch, pt_debug_morph_rest).  Included at the end of
// pt_image.hpp after pt_pose_host.hpp and pt_rig_host.hpp, inside pt_hip.hip's extern "C" block; not a translation unit.
//
// It takes the objects and their steps from those two files: ruleLaunch, morphRest, normalsInto, poseToHost, scratchStands and restInto of the
// pose; localsFromCaller, localsFromMix, rigMixTable, rigRun and rigRunLevels of the rig.  Nothing here is called by them.
//
// What a reader must know.  A timer refuses with "<name>: bad argument" before anything is enqueued, and ahead of any longer sentence about a
// pose of the wrong rule; it leaves *msBest alone unless it succeeds.  What is timed is what bestTime's `enqueue` puts on the plan's stream,
// which is idle before the first repetition; every repetition writes the same bits, so the object answers afterwards as it did before.  The
// pose timers work in the pose's scratch copy, never in the plan's working copies.
namespace {

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

// what the timers over a pose's records ask first: a live pose, somewhere to put the time, a repetition, records present and of the pose's size
bool recordsTimable(pt_pose* P, const float* xforms, size_t xformBytes, int reps, const float* msBest) {
    return poseLive(P) && msBest && reps >= 1 && xforms && P->nParts >= 1 && xformBytes == (size_t)P->nParts * RECORD_BYTES;
}
// and the rig's two: a live rig with a joint
bool rigTimable(pt_rig* G, int reps, const float* msBest) { return rigLive(G) && msBest && reps >= 1 && G->n >= 1; }

// the scratch copy holds the whole rest pose again, the records `xforms` lie in dX and the plan's stream is idle: what pt_debug_pose_scratch reads
// after a launch of the pose's rule into the scratch copy is that launch's work alone
int scratchAtRest(pt_pose* P, const float* xforms) {
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipSetDevice(P->device));
    if (const int rc = P->scratchReady ? restInto(P, P->dScratch) : scratchStands(P)) return rc;      // (a copy made now holds the rest pose already)
    const size_t bytes = (size_t)P->nParts * RECORD_BYTES;
    HIP_TRY(P->dX.ensure(bytes));
    HIP_TRY(hipMemcpyAsync(P->dX, xforms, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// the three rule timers after their checks: the statement `which` of the pose's rule from the rest pose into the scratch copy
int ruleTime(pt_pose* P, const float* xforms, int which, int reps, const char* who, float* msBest) {
    if (const int rc = scratchAtRest(P, xforms)) return rc;
    return bestTime(P->plan->stream, reps, who, [&] { return ruleLaunch(P, P->dRest, P->dScratch, which) == hipSuccess; }, msBest);
}

}  // namespace

// the device time of one pose launch (the best of reps), into the pose's scratch copy
int pt_debug_pose_time(pt_pose* P, const float* xforms, size_t xformBytes, int which, int reps, float* msBest) {
    if (!recordsTimable(P, xforms, xformBytes, reps, msBest) || (which != PT_POSE_PER_QUAD && which != PT_POSE_PER_TRIANGLE)) return fail(PT_ERR_ARG, "pt_debug_pose_time: bad argument");
    if (P->rule == RULE_SKIN_DQ) return fail(PT_ERR_ARG, "pt_debug_pose_time: a DQ pose has no part table (pt_debug_skin_dq_time times its kernels)");
    if (P->rule == RULE_SKIN) return fail(PT_ERR_ARG, "pt_debug_pose_time: a skinned pose has no part table (pt_debug_skin_time times its kernels)");
    return ruleTime(P, xforms, which, reps, "pt_debug_pose_time", msBest);
}

// the device time of one skin launch (the best of reps), into the pose's scratch copy
int pt_debug_skin_time(pt_pose* P, const float* xforms, size_t xformBytes, int which, int reps, float* msBest) {
    if (!recordsTimable(P, xforms, xformBytes, reps, msBest) || !hasBones(P) || (which != PT_SKIN_PER_QUAD && which != PT_SKIN_PER_CORNER))
        return fail(PT_ERR_ARG, "pt_debug_skin_time: bad argument");
    if (P->rule == RULE_SKIN_DQ) return fail(PT_ERR_ARG, "pt_debug_skin_time: a DQ pose blends no matrices (pt_debug_skin_dq_time times its kernels)");
    return ruleTime(P, xforms, which, reps, "pt_debug_skin_time", msBest);
}

// the device time of the two launches of a DQ pose, records then corners (the best of reps), into the pose's scratch copy
int pt_debug_skin_dq_time(pt_pose* P, const float* xforms, size_t xformBytes, int reps, float* msBest) {
    if (!recordsTimable(P, xforms, xformBytes, reps, msBest) || P->rule != RULE_SKIN_DQ) return fail(PT_ERR_ARG, "pt_debug_skin_dq_time: bad argument");
    return ruleTime(P, xforms, 0, reps, "pt_debug_skin_dq_time", msBest);
}

// the pose's scratch copy as the last pt_pose_triangles / pt_debug_pose_time / pt_debug_skin_time / pt_debug_skin_dq_time left it
int pt_debug_pose_scratch(pt_pose* P, float* trisOut, size_t triBytes) {
    const bool live = poseLive(P);
    if (!live || !trisOut || !P->scratchReady || triBytes != (size_t)P->nTris * TRI_BYTES) return fail(PT_ERR_ARG, "pt_debug_pose_scratch: bad argument");
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipSetDevice(P->device));
    if (P->nTris) HIP_TRY(hipMemcpyAsync(trisOut, P->dScratch, triBytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PT_OK;
}

// the device time of one k_morph_corners launch (the best of reps) under the given weights, into the morphed rest pose
int pt_debug_morph_time(pt_pose* P, const float* weights, size_t weightBytes, int reps, float* msBest) {
    const bool live = poseLive(P);
    if (!msBest || reps < 1 || ptp::checkMorphWeights(live, live && P->nTargets, weights, weightBytes, live ? P->nTargets : 0).code)
        return fail(PT_ERR_ARG, "pt_debug_morph_time: bad argument");
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipSetDevice(P->device));
    HIP_TRY(hipMemcpyAsync(P->dMorphW, weights, (size_t)P->nTargets * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return bestTime(st, reps, "pt_debug_morph_time", [&] {
        return ptMorphLaunch(P->dRest, P->dMorphCorner, P->dMorphRow, P->dMorphEntry, P->dMorphW, P->nAffected, P->dMorphRest, st) == hipSuccess;
    }, msBest);
}

// the morph kernel alone, under the weights last set (launched also when every weight is zero), and the morphed rest pose downloaded
int pt_debug_morph_rest(pt_pose* P, float* trisOut, size_t triBytes) {
    const bool live = poseLive(P);
    if (!live || !P->nTargets || !trisOut || triBytes != (size_t)P->nTris * TRI_BYTES) return fail(PT_ERR_ARG, "pt_debug_morph_rest: bad argument");
    const hipStream_t st = P->plan->stream;
    HIP_TRY(hipSetDevice(P->device));
    if (const int rc = morphRest(P, P->weights.data())) return rc;
    if (P->nTris) HIP_TRY(hipMemcpyAsync(trisOut, P->dMorphRest, triBytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PT_OK;
}

// the pose under the weights last set and the rule's normals into the scratch copy once, then the device time of the faces launch plus the
// chosen statement of the gather over it (the best of reps)
int pt_debug_normals_time(pt_pose* P, const float* xforms, size_t xformBytes, int which, int reps, float* msBest) {
    if (!recordsTimable(P, xforms, xformBytes, reps, msBest) || !P->hasNormals || (which != PT_NORMALS_PER_VERTEX && which != PT_NORMALS_PER_CORNER))
        return fail(PT_ERR_ARG, "pt_debug_normals_time: bad argument");
    std::vector<float> tris((size_t)P->nTris * TRI_FLOATS);
    if (const int rc = poseToHost(P, xforms, P->weights, 0, tris.data())) return rc;       // (the scratch copy holds the pose's rule's work afterwards; synchronised)
    // (a launch reads vertices and writes normals: every repetition gives the same bits)
    return bestTime(P->plan->stream, reps, "pt_debug_normals_time", [&] { return normalsInto(P, P->dScratch, (PtNormalsKernel)which) == 0; }, msBest);
}

// the device time of the rig's launches over the given locals, every level from the roots down (the best of reps), into dR
int pt_debug_rig_time(pt_rig* G, const float* locals, size_t localBytes, int reps, float* msBest) {
    if (!rigTimable(G, reps, msBest) || !locals || localBytes != (size_t)G->n * JOINT_BYTES) return fail(PT_ERR_ARG, "pt_debug_rig_time: bad argument");
    const float* at = localsFromCaller(G, locals);                // (selects the pose's device)
    if (!at) return PT_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(G->pose->plan->stream));
    // (a launch reads locals and parents' W and writes W and R: every repetition gives the same bits)
    return bestTime(G->pose->plan->stream, reps, "pt_debug_rig_time", [&] { return rigRun(G, at, G->dR) == 0; }, msBest);
}

// the device time of the mix's one launch over the given layers (the best of reps), into dLocals
int pt_debug_rig_mix_time(pt_rig* G, const pt_rig_layer* layers, size_t layerBytes, int reps, float* msBest) {
    if (!rigTimable(G, reps, msBest) ||
        ptp::checkRigMixLayers(ptp::RIG_MIX_LOCALS, nullptr, true, true, G->slots, layers, layerBytes, msBest, (size_t)G->n * JOINT_BYTES, G->n).code)      // (the layers' checks; no output here)
        return fail(PT_ERR_ARG, "pt_debug_rig_mix_time: bad argument");
    HIP_TRY(hipSetDevice(G->pose->device));                       // (ahead of bestTime's events, which are the first things enqueued)
    const PtRigMixTable T = rigMixTable(G, layers, layerBytes);
    // (a launch reads keys and masks and writes dLocals: every repetition gives the same bits)
    return bestTime(G->pose->plan->stream, reps, "pt_debug_rig_mix_time", [&] { return localsFromMix(G, T) != nullptr; }, msBest);
}

// the device time of the solve's one launch under the goals set (the best of reps): the given locals uploaded into dLocals and copied aside, the
// levels ahead of the solve once, then k_rig_ik reading the copy and writing dLocals
int pt_debug_rig_ik_time(pt_rig* G, const float* locals, size_t localBytes, int reps, float* msBest) {
    if (!rigTimable(G, reps, msBest) || !G->ikActive() || !locals || localBytes != (size_t)G->n * JOINT_BYTES) return fail(PT_ERR_ARG, "pt_debug_rig_ik_time: bad argument");
    const hipStream_t st = G->pose->plan->stream;
    const float* at = localsFromCaller(G, locals);                // (selects the pose's device)
    if (!at) return PT_ERR_HIP;
    Dev<float> aside;
    HIP_TRY(aside.reset(localBytes));
    HIP_TRY(hipMemcpyAsync(aside, at, localBytes, hipMemcpyDeviceToDevice, st));
    if (const int rc = rigRunLevels(G, at, G->dR, 0, G->ikWindow.before)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    // (a launch reads the copy and W and writes dLocals: every repetition gives the same bits, those pt_rig_ik_locals downloads)
    return bestTime(st, reps, "pt_debug_rig_ik_time", [&] {
        return ptRigIkLaunch(G->dIkRows, G->dIkCons, G->dIkGoals, (int)G->nIk, G->dW, aside, G->dLocals, st) == hipSuccess;
    }, msBest);
}
