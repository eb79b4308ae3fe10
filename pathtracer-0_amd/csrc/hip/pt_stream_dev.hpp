// pt_stream_dev.hpp — the launches of the render kernels (included by pt_hip.hip behind pt_context.hpp; not a translation unit): the timed
// launches, the intersect launch as pt_launch_plan.hpp planned it (the compiled kernels and the code objects assembled from pt_extend_gfx950.s),
// the stream pool and the CU partition, StreamDev (the device side of the frame-stream scheduler of pt_stream_sched.hpp), and on top of it
// pump / flushStream, writeFrame, submitBatch and resolveTimes.
namespace {

int nextEventPair(pt_ctx::KT& k) {
    if (k.used == k.ev.size()) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return -1;
        k.ev.emplace_back(a, b);
    }
    return (int)k.used++;
}
#define TIMED_LAUNCH_ON(strm, kidx, ...)                                    \
    do {                                                                   \
        int ev_ = c->timing ? nextEventPair(c->kt[kidx]) : -1;            \
        if (ev_ >= 0) hipEventRecord(c->kt[kidx].ev[ev_].first, strm);     \
        __VA_ARGS__;                                                       \
        if (ev_ >= 0) hipEventRecord(c->kt[kidx].ev[ev_].second, strm);    \
    } while (0)
#define TIMED_LAUNCH(kidx, ...) TIMED_LAUNCH_ON(s, kidx, __VA_ARGS__)

struct PoolRun {            // host view of the path pool while a batch runs
    hipStream_t stream; State st; unsigned launched; int iter;      // launched: the host's upper bound on the slots an iteration visits
};
template <bool COUNT, typename StackT, int TPB, bool RARE>
void launchEP(pt_ctx* c, const PoolRun& pr, const DevScene& sc, const ptp::ExtendPlan& p) {
    hipLaunchKernelGGL((k_extend_persist<COUNT, StackT, TPB, RARE>), dim3(p.grid), dim3(TPB), p.lds, pr.stream, sc, pr.st, c->dQueue[pr.iter & 1], pr.iter, (int)pr.launched, c->dCtl, c->opt.refillMin,
                       c->opt.innerKeepEighths, p.nObjLds, p.noneMin);
}
// Kernel arguments of pt_extend_gfx950.s (offsets are written into the assembly)
struct EpAsmArgs {
    const void *nodes80, *tris, *roots, *G0, *G1; void* H; const unsigned* queue; Control* ctl;
    int ldsNodes, ldsTris, numObj, iter, nSlots, refillMin, keepEighths, noneMin;
    unsigned divM, divS, nWaves, mode;      // mode: 1 the fused trip, 0 the phase-voting loop
    void* dbg;                      // developer builds of the assembly (-DPT_ASM_DEBUG): 32 B per wave
    const void* ellip; int numEllip, nodeStride;      // EllipRec array (rotation matrices by k_frame_setup); bytes per node record (80 or 64)
    int groupShift, stackDepth;     // more than 8 BVHs: log2 of the objects per group box (the 64 group boxes follow the root records); levels of the traversal stacks (24-bit entries: where the byte array starts)
    void* HX;                       // State::HX of scenes whose ellipsoids carry texture-mapped materials, else null
};
static_assert(sizeof(EpAsmArgs) == 152 && offsetof(EpAsmArgs, HX) == 144 && offsetof(EpAsmArgs, ellip) == 120 && offsetof(EpAsmArgs, groupShift) == 136, "EpAsmArgs layout is part of the assembly");
static_assert(sizeof(EllipRec) == 128 && offsetof(EllipRec, rotated) == 32 && offsetof(EllipRec, R) == 48, "EllipRec layout is part of the assembly");
#ifndef PT_EXTEND_INC
#define PT_EXTEND_INC "pt_extend_hsaco.inc"
#endif
#include PT_EXTEND_INC              // the assembled code objects (build.py): pt_extend_hsaco_s16[], pt_extend_hsaco_p18[]

// One code object per variant, loaded when a launch first needs it (a stream uses one or two of the eighteen).  A variant that failed to load stays
// failed: the error is latched, nothing half-loaded is kept and later launches do not retry.
int loadAsmKernel(pt_ctx* c, int k) {
    if (c->asmFn[k]) return 0;
    if (!c->asmLoadError[k].empty()) return fail(PT_ERR_HIP, c->asmLoadError[k]);
    const void* images[18] = {pt_extend_hsaco_s16, pt_extend_hsaco_p18, pt_extend_hsaco_s16f, pt_extend_hsaco_p18f, pt_extend_hsaco_p24, pt_extend_hsaco_p24f,
                              pt_extend_hsaco_s16w, pt_extend_hsaco_p18w, pt_extend_hsaco_s16fw, pt_extend_hsaco_p18fw, pt_extend_hsaco_p24w, pt_extend_hsaco_p24fw,
                              pt_extend_hsaco_s16h, pt_extend_hsaco_p18h, pt_extend_hsaco_s16fh, pt_extend_hsaco_p18fh, pt_extend_hsaco_p24h, pt_extend_hsaco_p24fh};
    hipModule_t m = nullptr; hipFunction_t f = nullptr;
    hipError_t e = hipModuleLoadData(&m, images[k]);
    if (e == hipSuccess) e = hipModuleGetFunction(&f, m, "pt_extend_asm");
    if (e != hipSuccess) {
        if (m) hipModuleUnload(m);
        c->asmLoadError[k] = std::string("code object ") + std::to_string(k) + " of pt_extend_asm: " + hipGetErrorString(e);
        return fail(PT_ERR_HIP, c->asmLoadError[k]);
    }
    c->asmModule[k] = m; c->asmFn[k] = f;
    return 0;
}

// The plan of an intersect launch over the pool `pr` (pt_launch_plan.hpp) under the options o.  probes: the pool carries thickness probes (RAYTRACING == 0);
// fast: the relaxed reciprocal may be used
ptp::ExtendPlan planExtendFor(const pt_ctx* c, const ptp::Options& o, const PoolRun& pr, bool probes, bool fast) {
    ptp::PlanDevice dv; ptp::PlanCall call;
    dv.numCUs = c->numCUs; dv.streamsOnDevice = c->streamsOnDevice; dv.part = c->sExt != nullptr && pr.stream == c->sExt; dv.partEighths = c->cuPartitionBuilt;
    call.launched = pr.launched; call.probes = probes; call.fast = fast;
    return ptp::planExtend(c->built, o, dv, call);
}

// true: launched.  false: the load or the launch failed; c->asmError says why (loud: pump() fails, no silent fallback)
bool launchExtendAsm(pt_ctx* c, const PoolRun& pr, const ptp::ExtendPlan& p) {
    if (loadAsmKernel(c, p.variant)) { c->asmError = "hand-written intersect kernel: " + g_err; return false; }
    EpAsmArgs a{};
    a.nodes80 = c->dNodes80; a.tris = c->dTris; a.roots = c->dRoots; a.G0 = pr.st.G0; a.G1 = pr.st.G1; a.H = pr.st.H;
    a.queue = c->dQueue[pr.iter & 1]; a.ctl = c->dCtl;
    a.ellip = c->dEllip; a.numEllip = c->sc.numEllip; a.nodeStride = c->built.asmNodeStride; a.groupShift = c->asmGroupShift; a.stackDepth = c->built.stackDepth; a.HX = c->built.ellipMaps ? (void*)pr.st.HX : nullptr;
    a.numObj = c->sc.numObj; a.iter = pr.iter; a.nSlots = (int)pr.launched; a.refillMin = c->opt.refillMin; a.keepEighths = c->opt.innerKeepEighths;
    a.ldsNodes = p.ldsNodes; a.ldsTris = p.ldsTris; a.noneMin = p.noneMin; a.mode = p.mode; a.nWaves = p.nWaves; a.divM = p.divM; a.divS = p.divS;
#ifdef PT_ASM_DEBUG                  // developer builds only (scripts/build_variant.py -DPT_ASM_DEBUG): the per-wave debug records of the assembly
    {
        if (c->dAsmDbg.ensure(8192 * 64) != hipSuccess) return false;
        hipMemsetAsync(c->dAsmDbg, 0xff, 8192 * 64, pr.stream);
        a.dbg = c->dAsmDbg.p;
    }
#endif
    size_t asz = sizeof(a);
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &asz, HIP_LAUNCH_PARAM_END};
    const hipError_t e = hipModuleLaunchKernel(c->asmFn[p.variant], (unsigned)p.grid, 1, 1, (unsigned)p.tpb, 1, 1, (unsigned)p.lds, pr.stream, nullptr, extra);
    if (e != hipSuccess) { c->asmError = std::string("hipModuleLaunchKernel(pt_extend_asm): ") + hipGetErrorString(e); return false; }
    c->asmLaunches++;
    return true;
}

void launchExtendPersist(pt_ctx* c, const PoolRun& pr, const ptp::ExtendPlan& p) {
    DevScene sc = c->sc;
    sc.ldsNodes = p.ldsNodes; sc.ldsTris = p.ldsTris;
    const int tpb = p.tpb;
#define EP(COUNT, T, TPB) (p.rare ? launchEP<COUNT, T, TPB, true>(c, pr, sc, p) : launchEP<COUNT, T, TPB, false>(c, pr, sc, p))
#define EP_T(COUNT, T) do { if (tpb == 64) EP(COUNT, T, 64); else if (tpb == 128) EP(COUNT, T, 128); else if (tpb == 256) EP(COUNT, T, 256); else if (tpb == 512) EP(COUNT, T, 512); else EP(COUNT, T, 1024); } while (0)
    if (c->opt.countStats) { if (c->built.stackMode == 0) EP_T(true, short); else if (c->built.stackMode == 1) EP_T(true, Packed18); else EP_T(true, int); }
    else { if (c->built.stackMode == 0) EP_T(false, short); else if (c->built.stackMode == 1) EP_T(false, Packed18); else EP_T(false, int); }
#undef EP
#undef EP_T
}

// The intersect launch of one iteration over the pool `pr`, as planned; a hand-written kernel that failed to load or launch leaves the compiled one's
// launch behind it and its error in c->asmError
void launchExtend(pt_ctx* c, const PoolRun& pr, bool probes, bool fast) {
    const ptp::ExtendPlan p = planExtendFor(c, c->opt, pr, probes, fast);
    if (p.kernel == ptp::K_ASM) {
        if (!launchExtendAsm(c, pr, p)) {                         // the compiled kernel's plan where option 4 asked for the hand-written one
            ptp::Options compiled = c->opt; compiled.extendMode = 1;
            launchExtendPersist(c, pr, planExtendFor(c, compiled, pr, probes, fast));
        }
    }
    else if (p.kernel == ptp::K_PERSIST) launchExtendPersist(c, pr, p);
    else if (c->opt.countStats) hipLaunchKernelGGL(k_extend<true>, dim3(p.grid), dim3(BLOCK), p.lds, pr.stream, c->sc, pr.st, c->dQueue[pr.iter & 1], pr.iter, (int)pr.launched, c->dCtl);
    else hipLaunchKernelGGL(k_extend<false>, dim3(p.grid), dim3(BLOCK), p.lds, pr.stream, c->sc, pr.st, c->dQueue[pr.iter & 1], pr.iter, (int)pr.launched, c->dCtl);
}

// ------------------------------------------------------------------------------------------------ frame stream
// Which batch joins the running stream, the groups of iterations, the looks at the device's scheduler words and the retirements are decided in
// pt_stream_sched.hpp (pt_ctx::sched); what follows is the device side of it.

Batch streamBatch(const pt_ctx* c) {
    Batch b;
    b.W = c->W; b.H = c->H; b.nLocal = c->nLocal; b.nSlots = c->nSlotsImg; b.shardCount = c->shardCount;
    b.ringFrames = (unsigned)c->ringFrames; b.seeds = c->dSeeds; b.pixList = c->dPixList; b.pixXY = c->dPixXY; b.colbuf = c->dColbuf;
    // an adaptive stream runs on the compacted subsequence of the list; pixList then holds each entry's accumulator slot (k_accumulate_adaptive)
    if (c->adaptOn) { b.nLocal = c->adaptN; b.pixXY = c->dAdaptXY; b.pixList = c->dAdaptSlot; }
    if (b.nLocal >= 2) { const ptp::MagicDiv dm = ptp::magicDiv((unsigned)b.nLocal); b.divM = dm.m; b.divS = dm.s; }      // exact for every job < 2^31
    else { b.divM = 0; b.divS = 0; }
    return b;
}

// The streams of destroyed contexts are kept for later contexts of the process instead of being destroyed.  hipStreamDestroy right behind a long asynchronous run —
// hundreds of commands retired moments ago, the stream synchronised, the device synchronised — is where the HIP runtime (7.0.2 as bundled with torch) went on to
// decrement a counter inside the freed 920-byte stream object: a write after free that took the host heap with it about once in a thousand call sequences (glibc
// aborts, a std::bad_variant_access out of libamdhip64).  Found with a checking allocator (tools/canary_malloc.cpp), bisected to the scheduler that no longer
// synchronises the stream at every look, cured by never destroying a stream: 2500 sequences clean (profiles/r06_f_runtime_write_after_free.txt).  Streams are few
// and small.  key: the device, or (device + 1) * 100 + e (+ 50) for the CU-masked pair of the partition experiment.
std::mutex g_streamPoolLock;
std::vector<std::pair<int, hipStream_t>> g_streamPool;
bool pooledStream(int key, hipStream_t* out) {
    std::lock_guard<std::mutex> lk(g_streamPoolLock);
    for (size_t k = 0; k < g_streamPool.size(); k++)
        if (g_streamPool[k].first == key) { *out = g_streamPool[k].second; g_streamPool.erase(g_streamPool.begin() + (long)k); return true; }
    return false;
}
int takeStream(int device, hipStream_t* out) {
    if (pooledStream(device, out)) return 0;
    HIP_TRY(hipStreamCreateWithFlags(out, hipStreamNonBlocking));
    return 0;
}
void giveStream(int device, hipStream_t s) { std::lock_guard<std::mutex> lk(g_streamPoolLock); g_streamPool.emplace_back(device, s); }

// CU-masked streams of the spatial partition.  Bit k of a mask is CU k in the driver's order; whether consecutive bits walk the CUs of one XCD or the XCDs round-robin,
// the pattern ((k / 8) + (k % 8)) % 8 < e puts 4 e of every XCD's 32 CUs on the intersect side.
int ensurePartition(pt_ctx* c) {
    if (c->opt.cuPartition == c->cuPartitionBuilt) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->sExt) { hipStreamSynchronize(c->sExt); giveStream((c->device + 1) * 100 + c->cuPartitionBuilt, c->sExt); c->sExt = nullptr; }
    if (c->sShade) { hipStreamSynchronize(c->sShade); giveStream((c->device + 1) * 100 + 50 + c->cuPartitionBuilt, c->sShade); c->sShade = nullptr; }
    c->cuPartitionBuilt = 0;
    if (c->opt.cuPartition > 0) {
        const int words = (c->numCUs + 31) / 32;
        std::vector<uint32_t> mE((size_t)words, 0u), mS((size_t)words, 0u);
        for (int k = 0; k < c->numCUs; k++) {
            const bool ext = ((k / 8) + (k % 8)) % 8 < c->opt.cuPartition;
            (ext ? mE : mS)[(size_t)k / 32] |= 1u << (k % 32);
        }
        if (!pooledStream((c->device + 1) * 100 + c->opt.cuPartition, &c->sExt)) HIP_TRY(hipExtStreamCreateWithCUMask(&c->sExt, (uint32_t)words, mE.data()));
        if (!pooledStream((c->device + 1) * 100 + 50 + c->opt.cuPartition, &c->sShade)) HIP_TRY(hipExtStreamCreateWithCUMask(&c->sShade, (uint32_t)words, mS.data()));
        if (!c->evExt) { HIP_TRY(hipEventCreateWithFlags(&c->evExt, hipEventDisableTiming)); HIP_TRY(hipEventCreateWithFlags(&c->evShade, hipEventDisableTiming)); HIP_TRY(hipEventCreateWithFlags(&c->evHost, hipEventDisableTiming)); }
        c->cuPartitionBuilt = c->opt.cuPartition;
    }
    return 0;
}

// The device side of the frame-stream scheduler (pt_stream_sched.hpp): its launches, its waits and what a new stream needs.  The fields behind c are
// the submission at hand (submitBatch), else unset: its frame inputs, seeds and RAYTRACING == 0, the pool capacity and the ring rows a new stream gets
struct StreamDev {
    pt_ctx* c; const FrameIn* in = nullptr; const int32_t* seeds = nullptr; bool directNew = false; int capacity = 0, wantRing = 0;

    int launchIterations(int n, unsigned launched, int iter) {
        hipStream_t s = c->stream;
        { int rc = ensurePartition(c); if (rc) return rc; }
        const bool part = c->sExt != nullptr && s == c->ownStream;
        hipStream_t sx = part ? c->sExt : s, ss = part ? c->sShade : s;
        // the Parameters block the running stream was started with: a later pt_set_buffer(PT_BIND_PARAMS) only takes effect with the
        // next stream (the scheduler finishes this one first), so the remaining iterations keep their kernel variants and bounds
        const bool direct = c->hist.streamInputs().params[9] != 1.0f;
        const bool fastNow = c->streamFast;                           // the contract the running stream was started with
        const Batch b = streamBatch(c);
        if (part) { HIP_TRY(hipEventRecord(c->evHost, s)); HIP_TRY(hipStreamWaitEvent(sx, c->evHost, 0)); }      // what `s` holds (submission, revive, accumulate) comes first
        for (int k = 0; k < n; k++) {
            PoolRun pr; pr.stream = sx; pr.st = c->st; pr.launched = launched; pr.iter = (iter + k) & 0x3fffffff;
            TIMED_LAUNCH_ON(sx, 0, launchExtend(c, pr, direct, fastNow));
            if (part) { HIP_TRY(hipEventRecord(c->evExt, sx)); HIP_TRY(hipStreamWaitEvent(ss, c->evExt, 0)); }
#define SHADE_ARGS dim3(std::max(1, (int)((pr.launched + SHADE_BLOCK - 1) / SHADE_BLOCK))), dim3(SHADE_BLOCK), 0, ss, c->sc, b, c->dFc, pr.st, c->dQueue[pr.iter & 1], c->dQueue[(pr.iter + 1) & 1], pr.iter, (int)pr.launched, c->dCtl
            // kernel variant: transmissive materials present / statistics on / RAYTRACING == 0 / texture-mapped materials present
            // (T: index-stack encoding of the path state — 0 no transmissive material, 3 / 8 bits per slot)
#define SHADE_V(T, S, D, X) TIMED_LAUNCH_ON(ss, 1, hipLaunchKernelGGL((k_shade<T, S, D, X>), SHADE_ARGS))
#define SHADE_F(T, X) TIMED_LAUNCH_ON(ss, 1, hipLaunchKernelGGL((k_shade<T, false, false, X, true>), SHADE_ARGS))
            // (the relaxed numeric contract, pt_set_option 16: path tracing without statistics only; everything else keeps the exact kernels)
#define SHADE_S(T, D, X) do { if (c->opt.countStats) SHADE_V(T, true, D, X); else if (fastNow && !(D)) SHADE_F(T, X); else SHADE_V(T, false, D, X); } while (0)
#define SHADE_X(T, D) do { if (c->anyMaps) SHADE_S(T, D, true); else SHADE_S(T, D, false); } while (0)
            if (direct) SHADE_X(0, true);
            else if (c->niBits == 3) SHADE_X(3, false);
            else if (c->niBits == 8) SHADE_X(8, false);
            else if (c->niBits == 32) SHADE_X(32, false);
            else SHADE_X(0, false);
            if (part) { HIP_TRY(hipEventRecord(c->evShade, ss)); HIP_TRY(hipStreamWaitEvent(sx, c->evShade, 0)); }
        }
        if (part) HIP_TRY(hipStreamWaitEvent(s, c->evShade, 0));
        HIP_TRY(hipGetLastError());                                // a failed launch surfaces here, not as "did not drain"
        if (!c->asmError.empty()) { const std::string m = c->asmError; c->asmError.clear(); return fail(PT_ERR_HIP, m); }
        return 0;
    }
    int launchScan(const ptp::SchedScan& e) {
        ScanEnds ends{};
        for (int k = 0; k < 8; k++) ends.f[k] = e.f[k];
        ends.n = e.n;
        const int N = c->sched.poolActive;
        HIP_TRY(hipMemsetAsync(c->dCtl->busy, 0, sizeof(c->dCtl->busy), c->stream));
        hipLaunchKernelGGL(k_scan_inflight, dim3((N + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, c->st, N, ends, c->dCtl);
        return 0;
    }
    int launchSnapshot(int slot, unsigned seq) {
        pt_ctx::GroupPins& g = c->grp[slot];
        *g.stamp = 0;
        hipLaunchKernelGGL(k_snapshot, dim3(1), dim3(64), 0, c->stream, c->dCtl, g.h, g.stamp, seq);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    int landed(int slot, unsigned seq, bool wait, ptp::ControlView& v) {
        pt_ctx::GroupPins& g = c->grp[slot];
        // has the group's stamp arrived?  (k_snapshot writes it behind a system-scope fence after the snapshot; pinned coherent memory needs no synchronisation to be read)
        auto landed = [&]() { return *g.stamp == seq; };
        if (!landed()) {
            if (!wait) return 0;
            for (int spin = 0; spin < 4000 && !landed(); spin++) __builtin_ia32_pause();
            for (uint64_t n = 0; !landed(); n++) {
                std::this_thread::sleep_for(std::chrono::microseconds(n < 100 ? 20 : 100));
                if ((n & 1023) == 1023) {                              // every ~0.1 s: is the stream still working?  an idle stream without the stamp is a lost launch, an error a fault
                    const hipError_t q = hipStreamQuery(c->stream);
                    if (q != hipSuccess && q != hipErrorNotReady) return fail(PT_ERR_HIP, std::string("the wavefront stream failed: ") + hipGetErrorString(q));
                    if (q == hipSuccess && !landed()) return fail(PT_ERR_HIP, "the wavefront stream is idle but a group's snapshot never arrived (internal error)");
                }
            }
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        const Control& h = *g.h;
        v.nextJob = h.nextJob; v.qCount0 = h.qCount[0]; v.qCount32 = h.qCount[32];
        for (int k = 0; k < 4; k++) v.exhausted[k] = h.exhausted[k];
        for (int k = 0; k < 8; k++) v.busy[k] = h.busy[k];
        return 1;
    }
    int retire(const ptp::StreamEntry& e) {
        hipStream_t s = c->stream;
        Batch b = streamBatch(c);
        if (c->adaptOn) {
            TIMED_LAUNCH(3, hipLaunchKernelGGL(k_accumulate_adaptive, dim3((c->adaptN + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, b, c->dImage[e.image], c->dStats, e.f0, e.nFrames, e.firstFrame));
            HIP_TRY(hipGetLastError());
            return 0;
        }
        int gridA = (c->nSlotsImg + BLOCK - 1) / BLOCK;
        if (c->recordMoments && e.image == c->hist.image()) TIMED_LAUNCH(3, hipLaunchKernelGGL(k_accumulate_moments, dim3(gridA), dim3(BLOCK), 0, s, b, c->dFc, c->dImage[e.image], c->dStats, e.f0, e.nFrames, e.firstFrame));
        else TIMED_LAUNCH(3, hipLaunchKernelGGL(k_accumulate, dim3(gridA), dim3(BLOCK), 0, s, b, c->dFc, c->dImage[e.image], e.f0, e.nFrames, e.firstFrame));
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // every job retires within SAMPLE_RES * ceil(MAX_BOUNCES) iterations of being started
    uint64_t itersPerJob() const { const float* P = c->hist.streamInputs().params; return (uint64_t)(std::ceil(P[4]) * std::ceil(P[5]) + 1); }
    int didNotDrain() { return fail(PT_ERR_HIP, "wavefront scheduler did not drain (internal error)"); }

    int sceneReady() {
        if (c->sceneDirty) { const int rc = buildScene(c); if (rc) return rc; }
        if (directNew && c->anySubsurface) {
            if (c->sc.numObj > FL_PROBE_OBJ_MAX + 1) return fail(PT_ERR_UNSUPPORTED, "directDiffuse with subsurface materials supports at most 65536 objects (BVHs)");
            if (c->ambiguousTriObj) return fail(PT_ERR_SCENE, "directDiffuse with subsurface materials needs every triangle to belong to one BVH (hit.parentID, frag.glsl:573)");
        }
        return 0;
    }
    int openStream(int pool) {
        hipStream_t s = c->stream;
        if (const int rc = ensurePool(c, capacity)) return rc;
        if (c->ringFrames < wantRing) {
            HIP_TRY(hipStreamSynchronize(s));
            c->ringFrames = 0;
            HIP_TRY(c->dColbuf.reset((size_t)wantRing * (size_t)c->nSlotsImg * 16));
            HIP_TRY(c->dSeeds.reset((size_t)wantRing * 4));
            HIP_TRY(c->hSeeds.reset((size_t)wantRing * 4));
            c->ringFrames = wantRing;
        }
        c->hist.streamStarted(*in); *c->hFrameIn = *in; c->streamFast = c->opt.fastContract;
        HIP_TRY(hipMemcpyAsync(c->dFrameIn, c->hFrameIn, sizeof(FrameIn), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_frame_setup, dim3(1), dim3(64), 0, s, c->sc, c->dFrameIn, c->dFc, c->dEllip);
        hipLaunchKernelGGL(k_init_control, dim3(1), dim3(1), 0, s, c->dCtl);
        HIP_TRY(hipMemsetAsync(c->st.G1, 0, (size_t)pool * 16, s));       // every slot dead
        return 0;
    }
    int growPool(int from, int to) {
        HIP_TRY(hipMemsetAsync(c->st.G1 + from, 0, (size_t)(to - from) * 16, c->stream));      // the new slots are dead
        return 0;
    }
    int appendJobs(unsigned f0, int nFrames, unsigned nJobs, int mode, int N) {
        hipStream_t s = c->stream;
        for (int f = 0; f < nFrames; f++) c->hSeeds[(f0 + (unsigned)f) % (unsigned)c->ringFrames] = seeds[f];
        {
            unsigned r0 = f0 % (unsigned)c->ringFrames, n0 = std::min<unsigned>((unsigned)nFrames, (unsigned)c->ringFrames - r0);
            HIP_TRY(hipMemcpyAsync(c->dSeeds + r0, c->hSeeds + r0, (size_t)n0 * 4, hipMemcpyHostToDevice, s));
            if (n0 < (unsigned)nFrames) HIP_TRY(hipMemcpyAsync(c->dSeeds, c->hSeeds, (size_t)(nFrames - n0) * 4, hipMemcpyHostToDevice, s));
        }
        hipLaunchKernelGGL(k_submit, dim3(1), dim3(1), 0, s, c->dCtl, nJobs, mode, (unsigned)N);
        const Batch b = streamBatch(c);
#define REVIVE(T, F) TIMED_LAUNCH(2, hipLaunchKernelGGL((k_revive<T, F>), dim3((N + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, b, c->dFc, c->st, N, c->dCtl))
        const bool fastRevive = c->streamFast && !directNew && !c->opt.countStats;
        // (directDiffuse never touches the index stack: its k_shade variant is the one without it, and so is its path state — except that the pool of a
        //  scene with transmissive materials has the groups allocated, which k_revive<niBits> initialises)
        if (c->niBits == 3) { if (fastRevive) REVIVE(3, true); else REVIVE(3, false); }
        else if (c->niBits == 8) { if (fastRevive) REVIVE(8, true); else REVIVE(8, false); }
        else if (c->niBits == 32) { if (fastRevive) REVIVE(32, true); else REVIVE(32, false); }
        else { if (fastRevive) REVIVE(0, true); else REVIVE(0, false); }
#undef REVIVE
        c->hist.rendered(*in);                                    // the image's camera (include/pt_reproject.h)
        HIP_TRY(hipGetLastError());
        return 0;
    }
};

void countIterations(pt_ctx* c, uint64_t iters) { c->hostCnt[PT_CNT_ITERATIONS] += iters; c->hostCnt[PT_CNT_EXTEND_LAUNCHES] += iters; }
int pump(pt_ctx* c, ptp::PumpUntil until, int arg) {
    StreamDev dev{c};
    uint64_t iters = 0;
    const int rc = c->sched.pump(dev, until, arg, &iters);
    countIterations(c, iters);
    return rc;
}
int flushStream(pt_ctx* c) {
    if (c->sched.idle()) return 0;
    HIP_TRY(hipSetDevice(c->device));
    return pump(c, ptp::PUMP_IDLE, 0);
}

// pt_write_frame of a single context: FRAME from the whole host image; T from `stats` when given, else zeroed (where allocated); the camera recorded
int writeFrame(pt_ctx* c, const float* frame, const float* stats) {
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = flushStream(c))) return rc;
    if (c->dStats) {
        if (stats) { if ((rc = hostToShard(c, stats, c->dStats))) return rc; }
        else HIP_TRY(hipMemsetAsync(c->dStats, 0, (size_t)c->nSlotsImg * 16, c->stream));
    }
    recordCamera(c);
    return hostToShard(c, frame, c->dImage[c->hist.image()]);
}

int submitBatch(pt_ctx* c, int firstFrame, int nFrames, const int32_t* seeds, bool async) {
    if (nFrames < 1) return fail(PT_ERR_ARG, "n_frames must be >= 1");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    int rc;
    // parameter checks (scope: SURVEY.md §2)
    if (c->buf.params.size() < 12) return fail(PT_ERR_ARG, "Parameters (binding 4) not set");
    const float* P = c->buf.params.data();
    FrameIn fin{};
    currentInputs(c, fin);                                        // (a camera that is not set leaves it zeroed: the scene build refuses before anything reads it)
    if (P[10] != 0.0f) {                                          // DEBUG: no paths at all, one small kernel (frag.glsl:916-918)
        if ((int)P[2] != c->W || (int)(P[2] * P[3]) != c->H) return fail(PT_ERR_ARG, "Parameters.resolution / screenHratio do not match the FRAME image size given to pt_create");
        if ((rc = flushStream(c))) return rc;
        if (c->sceneDirty && (rc = buildScene(c))) return rc;
        if (c->built.stackDepth > 64) return fail(PT_ERR_SCENE, "DEBUG heat-map: BVH deeper than the 64-entry traversal stack");
        *c->hFrameIn = fin;
        HIP_TRY(hipMemcpyAsync(c->dFrameIn, c->hFrameIn, sizeof(FrameIn), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_frame_setup, dim3(1), dim3(64), 0, s, c->sc, c->dFrameIn, c->dFc, c->dEllip);
        c->hist.frameConstantsTaken();                                             // the frame constants on the device are no stream's any more
        const Batch b = streamBatch(c);
        DevScene dsc = c->sc; dsc.ldsNodes = 0; dsc.ldsTris = 0;                    // no LDS tile in this kernel
        hipLaunchKernelGGL(k_debug_heatmap, dim3((c->nLocal + 63) / 64), dim3(64), 0, s, dsc, b, c->dFc, c->dImage[c->hist.image()], firstFrame, nFrames);
        HIP_TRY(hipGetLastError());
        c->hist.rendered(fin);
        return 0;
    }
    if ((int)P[2] != c->W || (int)(P[2] * P[3]) != c->H) return fail(PT_ERR_ARG, "Parameters.resolution / screenHratio do not match the FRAME image size given to pt_create");
    // the loop bounds are floats in the shader (frag.glsl:820, :898); the slot's counters have 12 bits each
    if (!(P[4] >= 1.0f) || P[4] > 2047.0f) return fail(PT_ERR_ARG, "SAMPLE_RES must be in [1,2047]");
    if (!(P[5] > 0.0f) || P[5] > 4095.0f) return fail(PT_ERR_ARG, "MAX_BOUNCES must be in (0,4095]");
    size_t nJobs64 = (size_t)(c->adaptOn ? c->adaptN : c->nLocal) * (size_t)nFrames;
    if (nJobs64 >= (1ull << 31)) return fail(PT_ERR_ARG, "batch too large: pixels * frames must stay below 2^31 (split the batch)");
    // whether the running stream takes the batch, the pool, the groups of iterations and the retirements: the scheduler's (pt_stream_sched.hpp)
    ptp::SubmitReq q;
    q.firstFrame = firstFrame; q.nFrames = nFrames; q.image = c->hist.image(); q.nJobs = nJobs64; q.async = async;
    q.sceneDirty = c->sceneDirty; q.sameInputs = c->hist.streamHas(fin); q.sameContract = c->streamFast == c->opt.fastContract;
    q.ringFrames = c->ringFrames; q.wantRing = ptp::ringRows(nFrames, async, (size_t)c->nSlotsImg * 16, pt_ctx::IMAGES);
    q.poolSlots = c->opt.poolSlots; q.allocSlots = c->allocSlots;
    StreamDev dev{c, &fin, seeds, P[9] != 1.0f, ptp::newStreamCapacity(async, c->opt.poolSlots), q.wantRing};      // (RAYTRACING == 0: directDiffuse, frag.glsl:655-681, :911-912)
    uint64_t iters = 0;
    rc = c->sched.submit(dev, q, &iters);
    countIterations(c, iters);
    return rc;
}

int resolveTimes(pt_ctx* c) {
    for (auto& k : c->kt) {
        for (size_t i = 0; i < k.used; i++) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, k.ev[i].first, k.ev[i].second));
            k.ms += ms; k.launches++; k.each.push_back(ms);
        }
        k.used = 0;
    }
    return 0;
}

}  // namespace
