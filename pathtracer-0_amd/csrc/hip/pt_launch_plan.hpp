// pt_launch_plan.hpp — the host-only planning of an intersect launch (which kernel, block size, LDS split, grid and the constants the hand-written
// kernel is handed), of the path pool's size and of the frame ring's.  Pure integer arithmetic: no HIP runtime call and no context.  launchExtend and
// submitBatch (pt_stream_dev.hpp) fill the inputs from the context and act on the result; tests/c/launch_plan_check.cpp runs it on the CPU.
#pragma once
#include "pt_options.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdint>

// the node tile of a 256-thread block of the hand-written kernel when the context's streams share the GPU (planExtendAsm; the test builds it once with another value)
#ifndef PT_PLAN_TILE_SHARED
#define PT_PLAN_TILE_SHARED 16384
#endif

namespace ptp {

constexpr int PLAN_BLOCK = 256;                       // lanes of a k_extend block, and what pool sizes are rounded to (BLOCK of pt_kernels.hpp)
static_assert(POOL_SLOT_STEP == PLAN_BLOCK, "option 0 rounds the caller's pool to the blocks the planner sizes pools by");
constexpr size_t LDS_PER_CU = 160 * 1024;             // gfx950; one block may take all of it

// what the planner reads of the scene as built (SceneLayout::planScene, pt_scene_layout.hpp)
struct PlanScene {
    int nNodes = 0, nTriRecs = 0, numObj = 0, stackDepth = 1, stackMode = 2, asmNodeStride = 80;
    bool ellipMaps = false, asmEligible = false;
    int ldsNodes = 0, ldsTris = 0;                    // the tile of k_extend, which the layout sizes
};
struct PlanDevice {
    int numCUs = 256, streamsOnDevice = 1;
    bool part = false; int partEighths = 0;           // the launch goes to the spatial partition's intersect stream, which has this many eighths of the CUs
};
struct PlanCall {
    unsigned launched = 0;                            // the host's upper bound on the slots the launch visits
    bool probes = false;                              // the pool carries thickness probes (RAYTRACING == 0 of the running stream)
    bool fast = false;                                // the relaxed reciprocal may be used (the running stream's numeric contract)
};

using PlanOptions = Options;                          // the planner reads the options themselves (pt_options.hpp)

enum ExtendKernel { K_EXTEND = 0, K_PERSIST = 1, K_ASM = 2 };      // k_extend, k_extend_persist, pt_extend_asm
struct ExtendPlan {
    int kernel = K_EXTEND, tpb = PLAN_BLOCK, grid = 1; size_t lds = 0; int ldsNodes = 0, ldsTris = 0;
    int perCU = 0;                                    // blocks per CU the grid was sized for (the persistent kernels)
    // the persistent kernels: lanes waiting for their next object / retirement that make that phase worth a trip
    int noneMin = 0;
    // pt_extend_asm: the code object (loadAsmKernel), its main loop (1 the fused trip, 0 the phase-voting loop), x / nWaves as a multiplication
    int variant = 0; unsigned mode = 0, nWaves = 0, divM = 0, divS = 0;
    // k_extend_persist: the instance with the two rare features, the object roots it copies to LDS
    bool rare = false; int nObjLds = 0;
};

// x / d == mulhi(x, m) >> s for every x < 2^31: m = ceil(2^(31+l)/d), s = l - 1 with 2^(l-1) < d <= 2^l.  d >= 2
struct MagicDiv { unsigned m, s; };
inline MagicDiv magicDiv(unsigned d) {
    int l = 0;
    while ((1ull << l) < d) l++;
    return MagicDiv{(unsigned)(((1ull << (31 + l)) + d - 1) / d), (unsigned)(l - 1)};
}

// dynamic LDS of a k_extend block: [node tile][triangle tile][one traversal stack of ints per lane]
inline size_t kExtendLdsBytes(int ldsNodes, int ldsTris, int stackDepth) { return (size_t)ldsNodes * 64 + (size_t)ldsTris * 48 + (size_t)stackDepth * PLAN_BLOCK * 4; }

// The tile gives way to residency: when `want` blocks of fixed + cb bytes do not fit a CU, and a tile of at least minTile would, the tile shrinks to
// what does (rounded down to `align`).
inline size_t tileForResidency(size_t cb, size_t fixed, int want, size_t minTile, size_t align) {
    const size_t perBlock = LDS_PER_CU / (size_t)std::max(want, 1);
    if (fixed + cb + 16 > perBlock && perBlock > fixed + 16 + minTile) cb = std::min(cb, (perBlock - fixed - 16) & ~(align - 1));
    return cb;
}
// [node tile][triangle tile] in cb bytes: triangles only once every node is in; the block's LDS with its fixed part, rounded up to 16
inline void splitTile(ExtendPlan& p, const PlanScene& s, size_t cb, size_t nodeBytes, size_t fixed) {
    p.ldsNodes = (int)std::min<size_t>((size_t)s.nNodes, cb / nodeBytes);
    p.ldsTris = (p.ldsNodes == s.nNodes) ? (int)std::min<size_t>((size_t)s.nTriRecs, (cb - (size_t)p.ldsNodes * nodeBytes) / 48) : 0;
    p.lds = ((size_t)p.ldsNodes * nodeBytes + (size_t)p.ldsTris * 48 + fixed + 15) & ~(size_t)15;
}

// The hand-written kernel.  false: this launch is not one it takes (the plan is then the compiled kernel's, planExtend)
inline bool planExtendAsm(const PlanScene& s, const PlanOptions& o, const PlanDevice& dv, const PlanCall& call, ExtendPlan& p) {
    // (RAYTRACING == 0, directDiffuse: its rays are ordinary rayScene calls, and the thickness probes of subsurface materials — FL_PROBE: no offset, one BVH, no
    //  ellipsoids — are set up at the kernel's refill)
    if (!s.asmEligible || o.countStats || o.extendTpb != 256) return false;
    // Block size.  What bounds this kernel is its CU's instruction issue and vector-memory pipe together (profiles/r03_h_*): node steps served from
    // the LDS tile cost neither a tag lookup nor a round trip, and the tile is per BLOCK — the same bytes eight times over with 256-thread blocks.
    // Alone on its GPU the kernel therefore runs 2 blocks of 1024 threads per CU over a 32 KB tile instead of 8 x 256 over 8 KB (C3 +6.6 %, C4 +10 %,
    // C5 +7 %, C2 +-0).  When the context's streams share the GPU the small blocks win (their slots free one by one for the other stream's
    // shading blocks: 1024-thread blocks -4...7 %), and so they do for a launch too small to give every CU its two large blocks.
    const int cus = dv.part ? dv.numCUs * dv.partEighths / 8 : dv.numCUs;      // spatial partition: the kernel has its CUs to itself, but only those
    const bool sharedGpu = dv.streamsOnDevice > 1 && !dv.part;
    const bool lazyRoots = s.numObj > 8;                       // more than 8 BVHs: root records in LDS, tested when a BVH's turn comes (no per-lane distances)
    const size_t entryBytes = s.stackMode == 2 ? 3 : 2;        // traversal-stack entry in LDS: 16 bits (+ 2 in registers: Packed18), or 16 + 8 (24-bit entries)
    const size_t perLane = (lazyRoots ? 0 : (size_t)s.numObj * 4) + (size_t)s.stackDepth * entryBytes;      // root-box distances + traversal stack of one lane
    const size_t rootBytes = lazyRoots ? ((size_t)s.numObj + 64) * 32 : 0;      // the root records and the 64 group boxes of the per-ray cull (buildScene)
    const bool largeFits = 2 * (perLane * 1024 + rootBytes + 48 + 16384) <= LDS_PER_CU;      // two large blocks per CU with at least a 16 KB tile each (deep trees: stacks)
    const int TPB = o.asmTpb ? o.asmTpb : (!sharedGpu && dv.streamsOnDevice == 1 && largeFits && call.launched >= (uint64_t)cus * 2048 ? 1024 : 256);
    const int BPW = TPB / 256;                                  // how many 256-thread blocks one block stands for
    const size_t fixed = (lazyRoots ? rootBytes : (size_t)s.numObj * 4 * TPB) + 48 + (size_t)s.stackDepth * entryBytes * TPB;      // root-box distances (or root records), root references + ray cursor, traversal stacks
    if (fixed + 2048 > LDS_PER_CU) return false;
    // Blocks per CU and tile: alone on the GPU the kernel wants every wave slot (8 blocks of 256 threads, 8 KB tile).  When the context's streams
    // share the GPU (pt_create_multi with a device listed more than once) 6 blocks with a 16 KB tile are worth more: the two slots per SIMD it
    // leaves let the other stream's shading blocks run beside it instead of behind it (C3 +3.5 %, C4 +3 %, C5 +2.5 % over 8 blocks,
    // profiles/r03_d_blocks_per_cu_and_tile.txt) — unless the whole scene fits the small tile anyway (C2).
    const bool wholeSceneInSmallTile = (size_t)s.nNodes * (size_t)s.asmNodeStride + (size_t)s.nTriRecs * 48 <= 8192;
    const bool shareSlots = sharedGpu && !wholeSceneInSmallTile;
    const int maxBlocks = std::max(1, (o.extendMaxBlocksPerCU > 0 ? std::min(o.extendMaxBlocksPerCU, 8) : (shareSlots ? 6 : 8)) / BPW);
    const size_t tileWanted = o.extendCacheSet ? (size_t)o.extendCacheBytes : (size_t)(shareSlots ? PT_PLAN_TILE_SHARED : 8192) * (size_t)BPW;
    const size_t cb = tileForResidency(std::min<size_t>(tileWanted, LDS_PER_CU - fixed), fixed, maxBlocks, 2048, 16);
    p = ExtendPlan{};
    p.kernel = K_ASM; p.tpb = TPB;
    splitTile(p, s, cb, (size_t)s.asmNodeStride, fixed);
    p.perCU = std::max(1, std::min((int)(LDS_PER_CU / p.lds), maxBlocks));
    p.grid = std::max(1, std::min(cus * p.perCU, ((int)call.launched + TPB - 1) / TPB));
    const bool fastRcp = call.fast;
    p.variant = (s.stackMode == 2 ? (fastRcp ? 5 : 4) : (s.stackMode == 1 ? 1 : 0) + (fastRcp ? 2 : 0)) + (TPB == 1024 ? 6 : TPB == 512 ? 12 : 0);
    // main loop: the fused trip with fetch-at-decision, unless the whole scene sits in the LDS tile — then no fetch is worth hiding and the
    // phase-voting loop's fewer instructions per ray win (C2: 3.4 against 3.1 Gsamples/s, profiles/r03_c_*)
    const bool allInLds = p.ldsNodes == s.nNodes && p.ldsTris == s.nTriRecs;
    p.mode = o.asmLoop >= 0 ? (unsigned)o.asmLoop : (allInLds ? 0u : 1u);
    p.noneMin = o.noneMin;
    if (p.mode && !o.noneMinSet) p.noneMin = 2;      // the fused loop serves lanes that wait for their next BVH sooner (C3 +1.8 %, C5 +1 %, C4 / one stream +-0: profiles/r03_c_main_loops.txt (8))
    p.nWaves = (unsigned)p.grid * (unsigned)(TPB / 64);
    const MagicDiv dm = magicDiv(p.nWaves);           // x / nWaves == mulhi(x, divM) >> divS for x < 2^31 (nWaves >= 4)
    p.divM = dm.m; p.divS = dm.s;
    return true;
}

// The compiled persistent kernel
inline ExtendPlan planExtendPersist(const PlanScene& s, const PlanOptions& o, const PlanDevice& dv, const PlanCall& call) {
    ExtendPlan p;
    p.kernel = K_PERSIST;
    const int tpb = p.tpb = o.extendTpb;
    // LDS per block: [node tile][triangle tile][root-box distances][traversal stacks]; the tile takes what the fixed parts leave
    const size_t fixed = (size_t)std::min(s.numObj, 8) * tpb * 4 + (size_t)s.stackDepth * tpb * (s.stackMode == 2 ? 4 : 2) + 64 + 32 * 8 + (size_t)tpb * 4;     // (+ the per-lane slot numbers)     // + the LDS copies of up to 8 object roots
    const size_t avail = fixed < LDS_PER_CU ? LDS_PER_CU - fixed : 0;
    // a smaller node tile (down to 2 KB; 6 KB under blocks of 512 threads and more) if that lets every wave slot of the CU be used:
    // occupancy is worth more to this kernel than the last kilobytes of tile (8 instead of 6 waves per SIMD +9 %; tiles of 4, 8 and 16 KB
    // measure the same, profiles/r02_y_*)
    const int want = std::min(o.extendMaxBlocksPerCU > 0 ? o.extendMaxBlocksPerCU : 2048 / tpb, 2048 / tpb);
    const size_t cb = tileForResidency(std::min<size_t>((size_t)o.extendCacheBytes, avail), fixed, want, tpb >= 512 ? 6 * 1024 : 2 * 1024, 64);
    splitTile(p, s, cb, 64, fixed);
    // Blocks per CU of the grid = what is resident at once (LDS per block; 2048 threads per CU), capped by pt_set_option 8 (default: no cap).
    // All waves of the grid start within 1 µs of each other (per-wave stamps of a -DPT_WAVE_STAMPS build, scripts/wave_ends.py).
    // A grid LARGER than what is resident queues blocks behind the resident ones and is slower (with 512-thread blocks: 5-16 blocks per
    // CU on C3; C4 and C5, whose deeper traversal stacks then left room for 3 blocks only, lost 5 % and 13 % with 4).
    p.perCU = std::max(1, std::min((int)(LDS_PER_CU / std::max<size_t>(p.lds, 1)), 2048 / tpb));
    if (o.extendMaxBlocksPerCU > 0) p.perCU = std::min(p.perCU, o.extendMaxBlocksPerCU);
    const int maxUseful = ((int)call.launched + tpb - 1) / tpb;                  // never more blocks than 1 lane per ray
    p.grid = std::max(1, std::min(dv.numCUs * p.perCU, maxUseful));
    p.noneMin = o.noneMin;
    // the two rare features of the kernel are compiled into a variant of their own (their registers cost the common one spills):
    // thickness probes (RAYTRACING == 0 of the running stream, not of a later upload) and the side record of mapped ellipsoids
    p.rare = call.probes || s.ellipMaps;
    p.nObjLds = std::min(s.numObj, 8);
    return p;
}

// The intersect launch of one iteration.  pt_set_option 4: 0 one block per 256 lanes (k_extend), 1 persistent blocks (k_extend_persist), 2 the
// hand-written form of 1 for the launches it takes, 1 for the others
inline ExtendPlan planExtend(const PlanScene& s, const PlanOptions& o, const PlanDevice& dv, const PlanCall& call) {
    ExtendPlan p;
    if (o.extendMode == 0) {
        p.grid = std::max(1, (int)((call.launched + PLAN_BLOCK - 1) / PLAN_BLOCK));
        p.ldsNodes = s.ldsNodes; p.ldsTris = s.ldsTris; p.lds = kExtendLdsBytes(s.ldsNodes, s.ldsTris, s.stackDepth);
        return p;
    }
    if (o.extendMode == 2 && planExtendAsm(s, o, dv, call, p)) return p;
    return planExtendPersist(s, o, dv, call);
}

// ------------------------------------------------------------------------------------------------ the path pool and the frame ring (submitBatch)
constexpr size_t POOL_MIN = (size_t)1 << 20, POOL_MAX_SYNC = (size_t)1 << 22, POOL_MAX_ASYNC = (size_t)1 << 23;

// Slots of a new stream's pool.  poolSlots > 0: the caller's (pt_set_option 0)
inline int newStreamPool(size_t nJobs, bool async, int poolSlots) {
    if (poolSlots > 0) return poolSlots;
    // automatic pool (measured on C3, profiles/): 5/8 of the batch up to 2^23 when batches overlap
    // (a batch that drains: one slot per job up to 2^22 — a frame at a time, the reference's own loop, takes 16.0 instead of 19.2 ms per
    //  1080p frame with 2 M instead of 1 M slots, profiles/r02_m_frame_at_a_time_loop.txt: every job then runs from the first iteration)
    const size_t want = std::min<size_t>(std::max<size_t>(async ? nJobs * 5 / 8 : nJobs, POOL_MIN), async ? POOL_MAX_ASYNC : POOL_MAX_SYNC);
    return (int)((std::min<size_t>(want, std::max<size_t>(nJobs, PLAN_BLOCK)) + PLAN_BLOCK - 1) / PLAN_BLOCK * PLAN_BLOCK);
}
// ... and the slots allocated beyond them: room for the automatic pool of overlapped batches to grow while the stream runs (0: none)
inline int newStreamCapacity(bool async, int poolSlots) { return (async && poolSlots == 0) ? (int)POOL_MAX_ASYNC : 0; }

// A stream fed in small batches (the reference draws ONE frame per call) started with a small pool and lets it grow with the backlog: the size a
// pool of poolActive of allocSlots slots grows to now, with `outstanding` jobs not yet handed out, or 0 when it stays as it is
inline size_t grownPool(uint64_t outstanding, uint64_t jobsPerImage, int allocSlots, int poolActive) {
    size_t target = std::min<size_t>(std::max<size_t>(outstanding * 5 / 8, POOL_MIN), POOL_MAX_ASYNC);
    // an image is cheapest to finish two images later (pt_finish_image): keep an image's jobs worth several pool turnovers
    if (jobsPerImage) target = std::min<size_t>(target, std::max<size_t>((size_t)(jobsPerImage * 5 / 8), POOL_MIN));
    target = std::min<size_t>((target + PLAN_BLOCK - 1) / PLAN_BLOCK * PLAN_BLOCK, (size_t)allocSlots);
    const size_t cap = std::min<size_t>(POOL_MAX_ASYNC, (size_t)allocSlots);
    const bool grows = target > (size_t)poolActive + (size_t)poolActive / 4 || (target >= cap && target > (size_t)poolActive);      // (the last step to the largest pool may be a small one)
    return grows ? target : 0;
}

// Rows of the frame ring a batch of nFrames wants.  Overlapped: room for the batches of as many images as can be pending, and for callers that
// submit frame by frame to run ahead (at least 64 rows while they stay below 8 GB)
inline int ringRows(int nFrames, bool async, size_t rowBytes, int images) {
    if (!async) return nFrames;
    return std::max(images * nFrames, (int)std::min<size_t>(64, std::max<size_t>(1, ((size_t)8 << 30) / rowBytes)));
}

}  // namespace ptp
