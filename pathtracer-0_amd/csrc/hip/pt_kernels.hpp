// pt_kernels.hpp — the render kernels of the wavefront path tracer for MI355X (gfx950) and the records they take (included by pt_hip.hip inside
// its unnamed namespace, after pt_device.hpp; not a translation unit).  Kernel text only: no host function and no HIP runtime call, so that
// build.py's kernel_source_hash(), which covers this file, changes when a kernel changes and not when the host side does.
//
// Restates the per-pixel Monte-Carlo loop of the reference's fragment shader
// (/root/reference/src/shaders/frag.glsl:884-934) as a wavefront state machine:
//
//   k_frame_setup   uniform work hoisted out of the per-pixel loop: rotationMatrix(ROTATION)
//                   (:271-283) and the auto-focus ray (:901-906, identical for every pixel)
//   k_revive        starts jobs in dead path slots: job -> pixel, rngState = index + u_seed (:896), first camera ray
//                   (:899-908), trace() prologue (:811-818); slot i takes job i when a frame stream starts
//   k_extend_persist  rayScene (:548-653): per-object BVH traversal + ellipsoids; persistent blocks, LDS-staged top of
//                   the BVH, in-wave ray refill, one instruction stream per trip chosen by vote   [the hot kernel]
//                   (k_extend: the simple one-block-per-256-rays form, kept as the cross-check)
//   k_shade         trace() loop body (:823-879): material, index stack, chooseRay, absorption,
//                   emission, cut-off, throughput; sky on miss; sample end -> regenerate the next
//                   sample of the pixel-frame in place (serial rngState) or pull a
//                   new job with one block-aggregated atomic; finished pixel-frames go to `colbuf`;
//                   once job supply runs dry it packs the surviving slots into the next iteration's queue
//   k_scan_inflight is a live slot still on a frame of the oldest unaccumulated batch? (one pass per host poll)
//   k_accumulate    FRAME accumulation (:924-933) of one batch in u_frameCount order -> bit-identical to
//                   frame-at-a-time rendering
// and a host-side frame-stream scheduler (pt_stream_sched.hpp; submitBatch and StreamDev in pt_stream_dev.hpp are its device side): consecutive batches share one running
// path pool; the host launches iterations in groups and polls the device's scheduler words (Control).
//
// Path state is structure-of-arrays in float4 groups (16 B per lane per access = 1 KiB per wave
// instruction, fully coalesced).  No MFMA: the path is divergent scalar fp32 + pointer chasing.
constexpr int BLOCK = 256;
static_assert(BLOCK == EXTEND_BLOCK, "the layout sizes the LDS tile beside one traversal stack per lane of a block");
static_assert(BLOCK == ptp::PLAN_BLOCK, "the launch plan sizes k_extend's grid and LDS, and rounds the pool, by its blocks");
#ifndef SHADE_BLOCK_SIZE
#define SHADE_BLOCK_SIZE 256
#endif
constexpr int SHADE_BLOCK = SHADE_BLOCK_SIZE;     // threads per block of the shading kernel: one scheduler atomic per block per launch
constexpr int TILE_W = 32, TILE_H = 8;

// Path-state accesses stream through the caches once per launch — hundreds of MB per launch through 4 MB of L2 per XCD — while the OTHER stream's intersect
// kernel lives on the BVH's node and triangle lines staying there: every access of a state group (and of the per-frame colour rows) carries the non-temporal
// hint (`nt`: C3 +1.4 %, C4 +0.8 %, C5 +2.3 % with the hit-record stores of pt_extend_gfx950.s hinted too; profiles/r04_v_nontemporal_state.txt)
__device__ __forceinline__ float4 ldS(const float4* p) {
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void stS(float4* p, float4 v) {
    f32x4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<f32x4*>(p));
}

using ptp::FrameIn;               // the frame inputs (pt_image_history.hpp)

struct Control {            // device-resident scheduler words shared by the whole batch
    unsigned nextJob;       // next unassigned job
    // exhausted[(j+1)&3] is raised by the shading launch of iteration j when a job pull comes back empty (sticky).  A word is
    // written by iteration j-1 and read by iterations j and j+1 only, so every launch sees stable values:
    //   shading of iteration j writes the dense queue of surviving slots iff exhausted[j&3];
    //   iteration j reads its slots through that queue iff exhausted[(j-1)&3].
    unsigned exhausted[4];
    unsigned jobEnd;        // jobs submitted to the frame stream so far: ids [0, jobEnd) exist (k_submit)
    unsigned needRevive;    // k_submit -> k_revive: dead slots may take jobs again
    unsigned oldestBusy;    // k_scan_inflight: a live slot still works on the oldest unaccumulated batch
    unsigned long long cnt[8];   // PT_CNT_* (device side: segments, nodes, tritests, hitupd, samples, boxtests)
    unsigned qCount[64];    // entries of queue (j&1) at [32*(j&1)]: two words, 128 B apart
    unsigned long long dbg[16];  // developer build (-DPT_PHASE_STATS): trips and active lanes per phase of the intersect kernel
    unsigned busy[8];       // k_scan_inflight: busy[k] = a live slot still works on a frame of the k-th oldest unaccumulated batch
#if defined(PT_PHASE_STATS) || defined(PT_WAVE_STAMPS)
    unsigned long long waveEnd[8192];   // s_memrealtime (100 MHz) at which each wave of the last intersect launch finished
    unsigned long long waveStart[8192]; // ... and started
#endif
};
// pt_extend_gfx950.s reads these two by their byte offsets
static_assert(offsetof(Control, exhausted) == 4 && offsetof(Control, qCount) == 96, "Control layout is part of the hand-written kernel");
__device__ __forceinline__ bool queueIn(const Control* ctl, int iter) { return ctl->exhausted[(iter + 3) & 3] != 0; }

struct State {              // SoA path pool, float4 groups (see header comment)
    float4 *G0, *G1, *G2, *G3, *G4, *G5, *S0, *H;
    unsigned s0Plane;       // STK == 32 (the index stack as ten floats): S0 holds three planes of this many slots — stack slots 0-3, 4-7, 8-9
    uint2* J;               // (frame slot of the stream, accumulator slot) of the slot's job: written when the job starts, read when it ends
    float4* HX;             // (u, v, id) of the closest triangle behind an ellipsoid hit; only for scenes whose ellipsoids carry texture-mapped materials
    const float4* Z;        // 64 zero bytes, zeroed when the context allocates them and never written again: what a lane of k_shade reads in place of a group it does not need
};

// The frame stream: consecutive batches with the same frame inputs (Parameters, ORIGIN, ROTATION, MOUSE_POS) form ONE job
// sequence, job = streamFrame * nLocal + pixel, so that the path pool never drains between them.  Per-frame data (u_seed,
// the frame's colour row) live in rings of `ringFrames` rows indexed by streamFrame % ringFrames.
struct Batch {
    int W, H, nLocal, nSlots, shardCount;
    unsigned divM, divS;      // job / nLocal == mulhi(job, divM) >> divS for job < 2^31 (nLocal >= 2); divM == 0: nLocal == 1
    unsigned ringFrames;
    const int* seeds;         // device ring, ringFrames
    const int* pixList;       // device, nLocal: global pixel index in tile-major job order
    const unsigned* pixXY;    // device, nLocal: the same pixels as x | y << 16
    float4* colbuf;           // device ring, ringFrames * nSlots
};

// ------------------------------------------------------------------------------------------------ kernels

__global__ void k_frame_setup(DevScene sc, const FrameIn* in, FrameConst* fc, EllipRec* ellip) {
    __shared__ int stk[64];
    if (threadIdx.x != 0) return;
    const float* P = in->params;
    fc->screenSize = P[0]; fc->focalLength = P[1]; fc->resolution = P[2]; fc->screenHratio = P[3]; fc->SAMPLE_RES = P[4];
    fc->MAX_BOUNCES = P[5]; fc->BLUR = P[7]; fc->FOCAL_DISTANCE = P[8]; fc->AUTO_FOCUS = P[11];
    for (int k = 0; k < 3; k++) { fc->origin[k] = in->origin[k]; fc->rotation[k] = in->rotation[k]; fc->mouse[k] = in->mouse[k]; }
    auto rotM = [](float ax, float ay, float az, float* M) {      // rotateX * rotateY * (z != 0 ? rotateZ : I), row-major
        float cx = cos_(ax), sx = sin_(ax), cy = cos_(ay), sy = sin_(ay);
        float RX[9] = {1, 0, 0, 0, cx, sx, 0, -sx, cx};
        float RY[9] = {cy, 0, -sy, 0, 1, 0, sy, 0, cy};
        float RZ[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        if (az != 0.0f) { float cz = cos_(az), sz = sin_(az); RZ[0] = cz; RZ[1] = sz; RZ[3] = -sz; RZ[4] = cz; }
        float T[9];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) T[3 * i + j] = RX[3 * i] * RY[j] + RX[3 * i + 1] * RY[3 + j] + RX[3 * i + 2] * RY[6 + j];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) M[3 * i + j] = T[3 * i] * RZ[j] + T[3 * i + 1] * RZ[3 + j] + T[3 * i + 2] * RZ[6 + j];
    };
    rotM(in->rotation[0], in->rotation[1], in->rotation[2], fc->camRot);
    for (int i = 0; i < sc.numEllip; i++) {
        EllipRec& E = ellip[i];
        float rx = E.rot[0], ry = E.rot[1], rz = E.rot[2];
        E.rotated = length(v3(rx, ry, rz)) > 0.0f ? 1 : 0;       // frag.glsl:613
        if (E.rotated) {
            float cx = cos_(rx), sx = sin_(rx), cy = cos_(ry), sy = sin_(ry), cz = cos_(rz), sz = sin_(rz);
            float c0[3] = {cy * cz, cx * sz + cz * sx * sy, sx * sz - cx * cz * sy};      // rotateBack columns, :291-295
            float c1[3] = {-cy * sz, cx * cz - sx * sy * sz, cz * sx + cx * sy * sz};
            float c2[3] = {sy, -cy * sx, cx * cy};
            for (int r = 0; r < 3; r++) { E.RB[3 * r] = c0[r]; E.RB[3 * r + 1] = c1[r]; E.RB[3 * r + 2] = c2[r]; }
            rotM(rx, ry, rz, E.R);
        }
    }
    __threadfence();
    float mid = -1.0f;
    if (fc->AUTO_FOCUS == 1.0f) {                                  // :901-906
        DevScene s2 = sc; s2.ldsNodes = 0; s2.ldsTris = 0; s2.ellip = ellip;
        vec3 fwd = vecmat(v3(0.0f, 0.0f, 1.0f), fc->camRot);
        float t, u, v; int prim; Counters c;
        intersectScene<false>(s2, v3(in->origin[0], in->origin[1], in->origin[2]), fwd, stk, 1, nullptr, nullptr, t, u, v, prim, c);
        mid = (t < 1e25f) ? t : -1.0f;                             // result.distance (:641,:651)
    }
    fc->midToScene = mid;
    fc->focus = (fc->AUTO_FOCUS == 1.0f && mid > 0.0f) ? mid : fc->FOCAL_DISTANCE;
}

// Path state in memory (16 B per lane per group, consecutive lanes on consecutive slots):
//   G0 = O.xyz, D.x    G1 = D.yz, rngState, flags    G2 = throughput.rgb, index-stack codes (3-bit scenes)    G4 = sum over samples.rgb, pixel x | y << 16
//   G3 = incLight.rgb of the running sample, touched only while FL_INCNZ (pt_device.hpp)      J = (frame slot, accumulator slot), job start / job end only
//   G5 = RAY_ENTER_LOCATION, DISTANCE_TRAVELED and S0 = index-stack codes of an 8-bit scene: scenes with transmissive materials only
__device__ __forceinline__ void storeStack32(const State& st, unsigned i, const Path& p) {
    stS(st.S0 + i, make_float4(__uint_as_float(p.sk[0]), __uint_as_float(p.sk[1]), __uint_as_float(p.sk[2]), __uint_as_float(p.sk[3])));
    stS(st.S0 + st.s0Plane + i, make_float4(__uint_as_float(p.sk[4]), __uint_as_float(p.sk[5]), __uint_as_float(p.sk[6]), __uint_as_float(p.sk[7])));
    stS(st.S0 + 2 * (size_t)st.s0Plane + i, make_float4(__uint_as_float(p.sk[8]), __uint_as_float(p.sk[9]), 0.0f, 0.0f));
}
template <int STK>
__device__ __forceinline__ void storePath(const State& st, unsigned i, const Path& p) {
    stS(st.G0 + i, make_float4(p.O.x, p.O.y, p.O.z, p.D.x));
    stS(st.G1 + i, make_float4(p.D.y, p.D.z, __uint_as_float(p.rng), __uint_as_float(packFlags(p))));
    stS(st.G2 + i, make_float4(p.col.x, p.col.y, p.col.z, __uint_as_float(p.sc0)));
    stS(st.G3 + i, make_float4(p.inc.x, p.inc.y, p.inc.z, 0.0f));      // (job starts only; directDiffuse reads the group for every lane)
    stS(st.G4 + i, make_float4(p.sum.x, p.sum.y, p.sum.z, __uint_as_float(p.pix)));
    st.J[i] = make_uint2(p.fi, p.ls);
    if (STK) st.G5[i] = make_float4(p.enter.x, p.enter.y, p.enter.z, p.dist);
    if (STK == 8) st.S0[i] = make_float4(__uint_as_float(p.sc0), __uint_as_float(p.sc1), __uint_as_float(p.sc2), 0.0f);
    if (STK == 32) storeStack32(st, i, p);
}

// A new pixel-frame job (one fragment-shader invocation): fresh "globals" (SURVEY.md Q-1), rngState = index + u_seed.
// The caller follows up with startSample (kept separate so that k_shade has a single startSample site).
__device__ __forceinline__ void startJob(const Batch& b, const FrameConst& fc, unsigned job, Path& p) {
    unsigned fi = b.divM ? (__umulhi(job, b.divM) >> b.divS) : job;      // job / nLocal without an integer division
    unsigned k = job - fi * (unsigned)b.nLocal;
    unsigned xy = b.pixXY[k];
    const int seed = b.seeds[fi % b.ringFrames];                         // (both words of the job are asked for before either is used: one round trip)
    int px = (int)(xy & 0xffffu), py = (int)(xy >> 16);
    uint32_t index;
    pixelIndex(fc, b.W, b.H, px, py, index);
    p.pix = xy; p.fi = fi;
    p.ls = (b.shardCount == 1) ? (unsigned)(py * b.W + px) : k;
    p.rng = index + (uint32_t)seed;
    p.sum = v3(0.0f);
    p.sample = 0;
    p.applyAbs = false; p.inObj = false;
    p.enter = v3(0.0f); p.dist = 0.0f;
    p.sc0 = 0u; p.sc1 = 0u; p.sc2 = 0u;                         // every slot of the index stack 0.0 (dictionary code 0)
#pragma unroll
    for (int k = 0; k < 10; k++) p.sk[k] = 0u;
    p.stackSize = 0;
    p.incNZ = false; p.inc = v3(0.0f);
    p.alive = true;
}

// Every dead slot of the pool asks for a job (one scheduler atomic per block) and, if one is left, starts it: the start of
// a frame stream (all slots dead) and the restart after the pool ran dry between two batches.
template <int STK, bool FAST>
__global__ void __launch_bounds__(BLOCK) k_revive(Batch b, const FrameConst* fcp, State st, int nSlots, Control* ctl) {
    __shared__ unsigned sCnt[BLOCK / 64], sBase;
    const unsigned mode = ctl->needRevive;
    if (!mode) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned i = blockIdx.x * BLOCK + threadIdx.x;
    if (mode == 2u) {                                              // start of a stream: every slot is dead, slot i takes job i
        if (i >= (unsigned)nSlots || i >= ctl->jobEnd) return;
        const FrameConst& fc = *fcp;
        Path p;
        startJob(b, fc, i, p);
        startSample<STK, FAST>(fc, b.W, b.H, (int)(p.pix & 0xffffu), (int)(p.pix >> 16), p);
        storePath<STK>(st, i, p);
        st.H[i] = make_float4(1e30f, 0.0f, 0.0f, __int_as_float(PRIM_NONE));
        return;
    }
    const bool want = i < (unsigned)nSlots && !(__float_as_uint(st.G1[i].w) & FL_ALIVE);
    unsigned long long mask = __ballot(want);
    if (lane == 0) sCnt[wave] = (unsigned)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; w++) total += sCnt[w];
        sBase = total ? atomicAdd(&ctl->nextJob, total) : 0u;
    }
    __syncthreads();
    if (!want) return;
    unsigned off = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) off += (w < wave) ? sCnt[w] : 0u;
    const unsigned job = sBase + off + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
    if (job >= ctl->jobEnd) return;                               // stays dead
    const FrameConst& fc = *fcp;
    Path p;
    startJob(b, fc, job, p);
    startSample<STK, FAST>(fc, b.W, b.H, (int)(p.pix & 0xffffu), (int)(p.pix >> 16), p);
    storePath<STK>(st, i, p);
    st.H[i] = make_float4(1e30f, 0.0f, 0.0f, __int_as_float(PRIM_NONE));
}

// rayScene for every live path slot.  Dynamic LDS: [nodes 4*ldsNodes float4][tris 3*ldsTris float4][stack depth*BLOCK int]
template <bool COUNT>
__global__ void __launch_bounds__(BLOCK) k_extend(DevScene sc, State st, const unsigned* qIn, int iter, int nSlots, Control* ctl) {
    extern __shared__ float4 smem[];
    float4* ldsN = smem;
    float4* ldsT = smem + 4 * sc.ldsNodes;
    int* stkBase = reinterpret_cast<int*>(smem + 4 * sc.ldsNodes + 3 * sc.ldsTris);
    const unsigned* queue = queueIn(ctl, iter) ? qIn : nullptr;
    unsigned n = queue ? ctl->qCount[32 * (iter & 1)] : (unsigned)nSlots;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->qCount[32 * ((iter + 1) & 1)] = 0;     // cursor of the queue this iteration's shading may write
    if (blockIdx.x * BLOCK >= n) return;                       // whole block beyond the live range
    for (int k = threadIdx.x; k < 4 * sc.ldsNodes; k += BLOCK) ldsN[k] = sc.nodes[k];
    for (int k = threadIdx.x; k < 3 * sc.ldsTris; k += BLOCK) ldsT[k] = sc.tris[k];
    __syncthreads();
    unsigned q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n) return;
    unsigned i = queue ? queue[q] : q;
    float4 g0 = st.G0[i], g1 = st.G1[i];
    if (!(__float_as_uint(g1.w) & FL_ALIVE)) return;
    float t, u, v; int prim; Counters c;
    const unsigned fl = __float_as_uint(g1.w);
    intersectScene<COUNT>(sc, v3(g0.x, g0.y, g0.z), v3(g0.w, g1.x, g1.y), stkBase + threadIdx.x, BLOCK, ldsN, ldsT, t, u, v, prim, c,
                          (fl & FL_PROBE) != 0, probeObjOf(fl), st.HX ? st.HX + i : nullptr);
    st.H[i] = make_float4(t, u, v, __int_as_float(prim));
    if (COUNT) {
        atomicAdd(&ctl->cnt[PT_CNT_NODES], (unsigned long long)c.nodes);
        atomicAdd(&ctl->cnt[PT_CNT_TRITESTS], (unsigned long long)c.tritests);
        atomicAdd(&ctl->cnt[PT_CNT_HITUPD], (unsigned long long)c.hitupd);
        atomicAdd(&ctl->cnt[PT_CNT_BOXTESTS], (unsigned long long)c.boxtests);
    }
}

// Persistent, phase-selecting form of k_extend (the production intersect kernel).
//  * grid sized to the machine; every block stages the top of the BVH (and, when they fit, the triangles) into LDS
//    ONCE and then streams its share of the rays through it;
//  * per wave: a lane whose ray is finished takes the next ray of the wave's static range (ballot + prefix
//    popcount, no atomics) instead of idling until the slowest lane is done;
//  * every trip through the loop the wave issues ONE instruction stream — the inner-node step or the leaf step —
//    whichever more lanes are waiting for (ballot + popcount); the other lanes keep their entry for a later trip.
//    The kernel is VALU-issue bound (profiles/): what counts is lanes busy per issued instruction;
//  * the entry the reference would push last and pop next (the near child) stays in a register; only the far child
//    goes through the LDS stack.
// Per ray the sequence of visited nodes / tested triangles and every comparison are exactly rayBVH's (frag.glsl:
// 452-537): a lane never steps past a pending leaf, so `closest` evolves in the reference's order.
// `cur` = the entry this lane will process next (the virtual top of rayBVH's stack):
//   >= 0 and < CUR_NONE  inner node   |   < 0  leaf: first triangle record is -(cur+1)
//   CUR_NONE  ray alive, BVH of the current object exhausted   |   CUR_IDLE  lane has no ray
// (activity is folded into `cur` so that every wave-level vote is ONE v_cmp writing an SGPR pair)
//   CUR_DONE  ray finished, its hit record still in the lane's registers (stored at the wave's next refill)
// lanes set in a wave mask, as a 32-bit SCALAR: left to __popcll the compiler keeps the count 64 bits wide and compares two counts with
// v_cmp_*_u64 (there is no 64-bit scalar ordered compare) — six vector instructions per outer trip of the intersect kernel
__device__ __forceinline__ int wavePop(unsigned long long m) { int n; asm("s_bcnt1_i32_b64 %0, %1" : "=s"(n) : "s"(m) : "scc"); return n; }
constexpr int CUR_NONE = 0x7ffffffd;
constexpr int CUR_DONE = 0x7ffffffe;
constexpr int CUR_IDLE = 0x7fffffff;
// Traversal-stack entries (pending far children) live in LDS, one column per lane.  Their width decides how many blocks a CU holds:
//   short     trees below 32767 inner nodes / triangle records
//   Packed18  up to 131071: the low 16 bits in LDS, bits 16-17 in a per-lane shift register (two VGPRs, 2 bits per level, 32 levels)
//   int       anything larger
struct Packed18 {};
template <typename T> struct StackElem { typedef T type; };
template <> struct StackElem<Packed18> { typedef unsigned short type; };

#ifndef PT_EP_WAVES
#define PT_EP_WAVES 8        // waves per SIMD the register allocation must leave room for (8 blocks of 256 threads per CU)
#endif
template <bool COUNT, typename StackT, int TPB, bool RARE>
__global__ void __launch_bounds__(TPB, PT_EP_WAVES) k_extend_persist(DevScene sc, State st, const unsigned* qIn, int iter, int nSlots,
                                                       Control* ctl, int refillMin, int keepEighths, int nObjLds, int noneMin) {
    extern __shared__ float4 smem[];
    typedef typename StackElem<StackT>::type ElemT;
    constexpr bool PACKED = __is_same(StackT, Packed18);
    unsigned hiA = 0u, hiB = 0u;                                   // Packed18: bits 16-17 of the stacked entries, newest in hiA[1:0]
    float4* ldsN = smem;
    float4* ldsT = smem + 4 * sc.ldsNodes;
    // per-lane root-box distances (rayNode(o,d,root) of :468 depends on the ray only, so it is evaluated once per ray
    // when the lane takes the ray — all refilled lanes together — and only compared against `closest` later)
    float* rootDist = reinterpret_cast<float*>(smem + 4 * sc.ldsNodes + 3 * sc.ldsTris) + threadIdx.x;
    // the first nObjLds object roots (box + reference, 32 B each) are read by every refill and every next-object step: LDS copies
    float4* rootsL = reinterpret_cast<float4*>(reinterpret_cast<float*>(smem + 4 * sc.ldsNodes + 3 * sc.ldsTris) + nObjLds * TPB);
    // the slot a lane's ray came from is needed again only when the ray retires: parked in LDS, not in a register
    unsigned* slotL = reinterpret_cast<unsigned*>(rootsL + 2 * nObjLds) + threadIdx.x;
    ElemT* stk = reinterpret_cast<ElemT*>(reinterpret_cast<unsigned*>(rootsL + 2 * nObjLds) + TPB) + threadIdx.x;
    for (int k = threadIdx.x; k < 2 * nObjLds; k += TPB) rootsL[k] = reinterpret_cast<const float4*>(sc.roots)[k];
    for (int k = threadIdx.x; k < 4 * sc.ldsNodes; k += TPB) ldsN[k] = sc.nodes[k];
    for (int k = threadIdx.x; k < 3 * sc.ldsTris; k += TPB) ldsT[k] = sc.tris[k];
    __syncthreads();
    const unsigned* queue = queueIn(ctl, iter) ? qIn : nullptr;
    const unsigned n = queue ? ctl->qCount[32 * (iter & 1)] : (unsigned)nSlots;
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->qCount[32 * ((iter + 1) & 1)] = 0;     // cursor of the queue this iteration's shading may write
    [[maybe_unused]] const int lane = threadIdx.x & 63;
    const unsigned nWaves = gridDim.x * (TPB / 64), waveId = __builtin_amdgcn_readfirstlane(blockIdx.x * (TPB / 64) + (threadIdx.x >> 6));   // scalar: pos/end live in SGPRs
    const unsigned per = (((n + nWaves - 1) / nWaves) + 63u) & ~63u;       // static range of this wave, 64-aligned -> coalesced first fill
    unsigned pos = waveId * per;
    const unsigned end = min(pos + per, n);
    vec3 o = v3(0.0f), d = v3(0.0f), invD = v3(0.0f);
    float closest = 1e30f, hu = 0.0f, hv = 0.0f;
    int prim = PRIM_NONE, ob = 0, obEnd = 0, sp = 0, cur = CUR_IDLE;
    bool probe = false;
    unsigned slot = 0;
    Counters c;
#if defined(PT_PHASE_STATS) || defined(PT_WAVE_STAMPS)
    const unsigned long long tStart = __builtin_amdgcn_s_memrealtime();
#endif
#ifdef PT_PHASE_STATS
    unsigned long long ps[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // {trips, active lanes} x {refill, next-object/retire, inner, leaf}, outer trips, live lanes at outer trips
#define PS(k, lanes) do { ps[2 * (k)]++; ps[2 * (k) + 1] += (unsigned long long)(lanes); } while (0)
    unsigned long long pt_[5] = {0, 0, 0, 0, 0}, tPrev = __builtin_amdgcn_s_memtime();      // shader-clock cycles per phase: refill, next-object, inner, leaf, votes and the rest
#define PTIME(k) do { const unsigned long long tNow_ = __builtin_amdgcn_s_memtime(); pt_[k] += tNow_ - tPrev; tPrev = tNow_; } while (0)
#else
#define PS(k, lanes) do { } while (0)
#define PTIME(k) do { } while (0)
#endif
    for (;;) {
        // ---- refill idle lanes from the wave's range
        unsigned long long idle = __ballot(cur >= CUR_DONE);                // lanes without a ray in flight
        int nIdle = wavePop(idle);
        PS(4, 64 - nIdle);
        if (pos < end && nIdle >= refillMin) {                              // wave-uniform
            PS(0, min(nIdle, (int)(end - pos)));
            PTIME(4);
            if (cur >= CUR_DONE) {
                // the hit records of the rays that retired since the last refill leave together: one store instruction for all of them,
                // neighbouring slots of one refill generation close in time (the lanes retire out of order)
                if (cur == CUR_DONE) { st.H[*slotL] = make_float4(closest, hu, hv, __int_as_float(prim)); cur = CUR_IDLE; }
                // rank of this lane among the idle ones: v_mbcnt (set bits of the mask below the lane), no lane-mask registers
                unsigned q = pos + __builtin_amdgcn_mbcnt_hi((unsigned)(idle >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)idle, 0u));
                if (q < end) {
                    slot = queue ? queue[q] : q;
                    *slotL = slot;
                    float4 g0 = st.G0[slot], g1 = st.G1[slot];
                    // both groups in ONE round trip (left alone the compiler fetches the flags word first and the rest behind the branch)
                    asm volatile("" : "+v"(g0.x), "+v"(g0.y), "+v"(g0.z), "+v"(g0.w), "+v"(g1.x), "+v"(g1.y), "+v"(g1.z), "+v"(g1.w));
                    const unsigned fl = __float_as_uint(g1.w);
                    if (fl & FL_ALIVE) {
                        d = v3(g0.w, g1.x, g1.y);
                        probe = RARE && (fl & FL_PROBE) != 0;             // directDiffuse's thickness probe: rayBVH called directly (:668); only RAYTRACING == 0 makes them
                        o = probe ? v3(g0.x, g0.y, g0.z) : madd(d, 1e-4f, v3(g0.x, g0.y, g0.z));   // o = o + 1e-4*d  (:549)
                        invD = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
                        ob = probe ? probeObjOf(fl) : 0;
                        obEnd = probe ? ob + 1 : sc.numObj;
                        closest = 1e30f; hu = 0.0f; hv = 0.0f; prim = PRIM_NONE; sp = 0; cur = CUR_NONE;
                        for (int k = 0; k < nObjLds; k += 2) {              // two root boxes per packed-f32 test, like the two children of a node
                            const int kb = min(k + 1, nObjLds - 1);
                            const float4 a0 = rootsL[2 * k], a1 = rootsL[2 * k + 1], b0 = rootsL[2 * kb], b1 = rootsL[2 * kb + 1];
                            ObjRoot A, B;
                            A.bmin[0] = a0.x; A.bmin[1] = a0.y; A.bmin[2] = a0.z; A.bmax[0] = a0.w; A.bmax[1] = a1.x; A.bmax[2] = a1.y;
                            B.bmin[0] = b0.x; B.bmin[1] = b0.y; B.bmin[2] = b0.z; B.bmax[0] = b0.w; B.bmax[1] = b1.x; B.bmax[2] = b1.y;
                            float da, db;
                            rayBox2(o, invD, make_float4(A.bmin[0], B.bmin[0], A.bmin[1], B.bmin[1]), make_float4(A.bmin[2], B.bmin[2], A.bmax[0], B.bmax[0]),
                                    make_float4(A.bmax[1], B.bmax[1], A.bmax[2], B.bmax[2]), da, db);
                            rootDist[k * TPB] = da;
                            if (k + 1 < nObjLds) rootDist[(k + 1) * TPB] = db;
                        }
                    }
                }
            }
            pos += (unsigned)nIdle;
            nIdle = wavePop(__ballot(cur >= CUR_DONE));
            PTIME(0);
        }
        if (nIdle == 64) { if (pos >= end) break; continue; }
        // ---- lanes whose BVH is exhausted: next object (root box test :468), else ellipsoids + retire.  Like the two traversal
        // phases below this one is worth a trip only for enough lanes: it runs when noneMin lanes wait for it, or when it is the
        // most wanted of the three
        int nInner = wavePop(__ballot((unsigned)cur < (unsigned)CUR_NONE));   // cur in [0, CUR_NONE)
        int nLeaf = wavePop(__ballot(cur < 0));
        const int nNone = wavePop(__ballot(cur == CUR_NONE));
        if (nNone >= noneMin || (nNone > 0 && nNone >= nInner && nNone >= nLeaf)) {
            PS(1, nNone);
            PTIME(4);
            if (cur == CUR_NONE) {
                while (ob < obEnd) {
                    float rd; int rref;
                    if (ob < nObjLds) { rd = rootDist[ob * TPB]; rref = __float_as_int(rootsL[2 * ob + 1].z); }
                    else { const ObjRoot R = sc.roots[ob]; rd = rayBox(o, invD, R.bmin[0], R.bmin[1], R.bmin[2], R.bmax[0], R.bmax[1], R.bmax[2]); rref = R.ref; }
                    ob++;
                    if (COUNT) c.boxtests++;
                    if (rd > closest) continue;
                    if (rref == REF_EMPTY) { if (COUNT) c.nodes++; continue; }
                    cur = rref;
                    break;
                }
                if (cur == CUR_NONE) {                                      // all BVHs done: ellipsoids (:606-631), then retire the ray
                    for (int i = 0; i < (probe ? 0 : sc.numEllip); i++) {
                        const EllipRec& E = sc.ellip[i];
                        vec3 cc = v3(E.c[0], E.c[1], E.c[2]);
                        float t;
                        if (E.rotated) t = rayEllipsoid(vecmat(o, E.R), vecmat(d, E.R), cc, E.r, E.st[0], E.st[1], E.st[2]);
                        else t = rayEllipsoid(o, d, cc, E.r, E.st[0], E.st[1], E.st[2]);
                        if (t < closest) {
                            if (!(prim & PRIM_ELLIPSOID) || prim == PRIM_NONE) {                            // see intersectScene
                                if (RARE && st.HX) st.HX[*slotL] = make_float4(hu, hv, __int_as_float(prim), 0.0f);
                                hu = __int_as_float(prim);
                            }
                            closest = t; prim = PRIM_ELLIPSOID | i;
                        }
                    }
                    cur = CUR_DONE;
                }
            }
            nInner = wavePop(__ballot((unsigned)cur < (unsigned)CUR_NONE));
            nLeaf = wavePop(__ballot(cur < 0));
            PTIME(1);
        }
        PTIME(4);
        if (nInner >= nLeaf && nInner > 0) {
            // ---- inner-node steps (:521-532); repeated while most of the lanes that started the phase still sit on inner nodes
            const int keepGoing = (nInner * keepEighths) >> 3;
            do {
                PS(2, nInner);
                if ((unsigned)cur < (unsigned)CUR_NONE) {
                    float4 q0, q1, q2, q3;
                    loadNode2(sc, ldsN, cur, q0, q1, q2, q3);
                    if (COUNT) { c.nodes++; c.boxtests += 2; }
                    float Ld, Rd;
                    rayBox2(o, invD, q0, q1, q2, Ld, Rd);
                    const int lref = __float_as_int(q3.x), rref = __float_as_int(q3.y);
                    if (COUNT) { if (Ld < closest && lref == REF_EMPTY) c.nodes++; if (Rd < closest && rref == REF_EMPTY) c.nodes++; }
                    // :525-531 pushes the farther child first, so the nearer one (ties: the left one) is popped next
                    const bool rNear = Ld > Rd;
                    const int nearRef = rNear ? rref : lref, farRef = rNear ? lref : rref;
                    const float nearD = rNear ? Rd : Ld, farD = rNear ? Ld : Rd;
                    const bool nearOk = nearD < closest && nearRef != REF_EMPTY, farOk = farD < closest && farRef != REF_EMPTY;
                    if (nearOk) {
                        cur = nearRef;
                        if (farOk) {
                            stk[sp * TPB] = (ElemT)farRef; sp++;
                            if (PACKED) { hiB = __builtin_amdgcn_alignbit(hiB, hiA, 30); hiA = (hiA << 2) | (((unsigned)farRef >> 16) & 3u); }
                        }
                    } else if (farOk) {
                        cur = farRef;
                    } else if (sp > 0) {
                        cur = (int)stk[(--sp) * TPB];
                        if (PACKED) { cur = (int)(((unsigned)cur | (hiA << 16)) << 14) >> 14; hiA = __builtin_amdgcn_alignbit(hiB, hiA, 2); hiB >>= 2; }
                    } else {
                        cur = CUR_NONE;
                    }
                }
                nInner = wavePop(__ballot((unsigned)cur < (unsigned)CUR_NONE));
            } while (nInner > keepGoing);
            PTIME(2);
        } else if (nLeaf > 0) {
            // ---- leaf steps: one triangle of the pending leaf per step (:483-520); repeated while most lanes still have
            // triangles left in their leaf (the reference's builder can leave many triangles in one leaf)
            const int keepGoing = (nLeaf * keepEighths) >> 3;
            int nMore;
            do {
                PS(3, __popcll(__ballot(cur < 0)));
                bool more = false;
                if (cur < 0) {
                    int ti = -(cur + 1);
                    float4 t0, t1, t2;
                    loadTri(sc, ldsT, ti, t0, t1, t2);
                    unsigned idl = __float_as_uint(t2.y);
                    float t, u, v;
                    if (COUNT) c.tritests++;
                    rayTri(o, d, v3(t0.x, t0.y, t0.z), v3(t0.w, t1.x, t1.y), v3(t1.z, t1.w, t2.x), t, u, v);
                    if (t > 0.0f && t < closest) {                          // :489
                        closest = t; hu = u; hv = v; prim = (int)(idl & 0x7fffffffu);
                        if (COUNT) c.hitupd++;
                    }
                    if (idl >> 31) {                                        // last triangle of the leaf: this node is done
                        if (COUNT) c.nodes++;
                        if (sp > 0) {
                            cur = (int)stk[(--sp) * TPB];
                            if (PACKED) { cur = (int)(((unsigned)cur | (hiA << 16)) << 14) >> 14; hiA = __builtin_amdgcn_alignbit(hiB, hiA, 2); hiB >>= 2; }
                        } else cur = CUR_NONE;
                    } else {
                        cur = cur - 1;                                      // next triangle record of the same leaf
                        more = true;
                    }
                }
                nMore = wavePop(__ballot(more));
            } while (nMore > keepGoing);
            PTIME(3);
        }
    }
    if (cur == CUR_DONE) st.H[*slotL] = make_float4(closest, hu, hv, __int_as_float(prim));      // the rays that retired after the last refill
    if (COUNT) {
        atomicAdd(&ctl->cnt[PT_CNT_NODES], (unsigned long long)c.nodes);
        atomicAdd(&ctl->cnt[PT_CNT_TRITESTS], (unsigned long long)c.tritests);
        atomicAdd(&ctl->cnt[PT_CNT_HITUPD], (unsigned long long)c.hitupd);
        atomicAdd(&ctl->cnt[PT_CNT_BOXTESTS], (unsigned long long)c.boxtests);
    }
#ifdef PT_PHASE_STATS
    if (lane == 0) { for (int k = 0; k < 10; k++) atomicAdd(&ctl->dbg[k], ps[k]); for (int k = 0; k < 5; k++) atomicAdd(&ctl->dbg[10 + k], pt_[k]); }
#endif
#if defined(PT_PHASE_STATS) || defined(PT_WAVE_STAMPS)
    if (lane == 0 && waveId < 8192) { ctl->waveEnd[waveId] = __builtin_amdgcn_s_memrealtime(); ctl->waveStart[waveId] = tStart; }
#endif
#undef PS
#undef PTIME
}

// trace() loop body + sample/job bookkeeping for every live path slot.
// Thread t of a block handles queue position (or slot) blockIdx*256 + t: every access to the path state is 16 B per lane at
// consecutive addresses.  (An earlier form sorted the block's slots by outcome — hit / miss / dead — through LDS so that waves
// ran one instruction stream each; once the kernel had become memory-bound the permuted accesses cost more than the
// divergence saved: 2-4 % per step on C2-C5, profiles/; likewise the dense LDS-listed pass that used to compute the camera
// rays of new samples for the whole block.)
// fcp is __restrict__: nothing the kernel stores aliases the frame constants, so their reads stay scalar loads after its first store; without it
// each read in a divergent branch (bounce budget, SAMPLE_RES, the camera) became a vector load with a wait of its own (profiles/r07_shade_load_tiers.txt).
template <int STK, bool STATS, bool DIRECT, bool TEX, bool FAST = false>
// (the texture-map variants are asked for 5 waves per SIMD: left alone the compiler spends 104-110 registers on them, 4 waves; at 96 it spills two and a
//  scene with a map on every material gains 3 %: profiles/r05_k_textured_materials.txt.  The float-stack variant would spill ten: left alone.)
__global__ void __launch_bounds__(SHADE_BLOCK, (TEX && !STATS && STK != 32) ? 5 : 1) k_shade(DevScene sc, Batch b, const FrameConst* __restrict__ fcp, State st, const unsigned* qIn, unsigned* qOut, int iter,
                                                 int nSlots, Control* ctl) {
    constexpr bool TRANS = STK != 0;
    __shared__ unsigned sCntA[SHADE_BLOCK / 64], sCntB[SHADE_BLOCK / 64], sBase;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long ltMask = (1ull << lane) - 1ull;
    const FrameConst& fc = *fcp;
    const unsigned* queue = queueIn(ctl, iter) ? qIn : nullptr;
    const unsigned n = queue ? ctl->qCount[32 * (iter & 1)] : (unsigned)nSlots;
    const bool writeQueue = ctl->exhausted[iter & 3] != 0;        // job supply ran dry before this iteration: pack the survivors
    const unsigned jobEnd = ctl->jobEnd;
    if (writeQueue && blockIdx.x == 0 && threadIdx.x == 0) ctl->exhausted[(iter + 1) & 3] = 1u;     // sticky, also through an empty launch
    if (blockIdx.x * SHADE_BLOCK >= n) return;                           // the grid is sized by the host's last known bound
    // ---- 1. the slot and its state, in two round trips — the kernel's critical path is memory round trips, not bytes: (G2 G1 G0 H, the index stack),
    // then, once the flags and the hit record have said what the segment ends, (G3 G5 G4 J), which is still in flight under the job pull's barrier.
    const unsigned q = blockIdx.x * SHADE_BLOCK + threadIdx.x;
    const bool valid = q < n;
    const unsigned i = valid ? (queue ? queue[q] : q) : 0u;
    float4 g0 = make_float4(0, 0, 0, 0), g1 = g0, g2 = g0, g3 = g0, g4 = g0, h = g0, s0 = g0, s1 = g0, s2 = g0, g5 = g0;
    // Path tracing decides BEFORE it shades whether the segment ends its sample (segmentEndsSample: the hit record, the throughput and the bounce count say so):
    // the sum over the job's samples (G4, 16 B) and the job words (J) are then fetched by the lanes whose sample / job ends only — a segment in four — and the job
    // pull runs while those loads and the shading records are on their way.  directDiffuse learns it from the material (a subsurface hit goes on as a probe): old order.
    constexpr bool EARLY = !DIRECT;
    // ONE_TRIP: the groups that only some lanes need — incLight (G3) while FL_INCNZ, the medium-entry group (G5), the sum (G4) at a sample's end, the job
    // words (J) at a job's end — are loaded by EVERY live lane in one batch, without a branch: a lane that does not need a group reads the context's
    // zero block (st.Z) in its place.  A load under `if (flag)` meets the register's initial value in a phi at the end of the `if`, and the compiler
    // waits for the load there: four flags were four round trips in a row, before the job pull's barrier, for every wave with one such lane (nearly
    // all).  With the address selected instead there is nothing to merge, and the wait moves to the first use: G3 and G5 rely on the block's zeros
    // (their initial value), G4 and J are used and stored under sampleDone / jobDone only.  The instantiations held to 96 registers by the launch
    // bounds (texture maps) have none to spare for four loads in flight — they spill — and keep the predicated loads.
    constexpr bool ONE_TRIP = EARLY && !(TEX && !STATS && STK != 32);
    if (valid) {
        // (G2 first: in the order G1 G0 H G2 the compiler issues G2 behind the wait for G1 — the flags' copy out of the `if` — a round trip later)
        g2 = ldS(st.G2 + i); g1 = ldS(st.G1 + i); g0 = ldS(st.G0 + i); h = ldS(st.H + i);
        if (!EARLY) g4 = ldS(st.G4 + i);
        if (STK == 8 || STK == 32) s0 = ldS(st.S0 + i);
        if (STK == 32) { s1 = ldS(st.S0 + st.s0Plane + i); s2 = ldS(st.S0 + 2 * (size_t)st.s0Plane + i); }
        if (DIRECT) g3 = ldS(st.G3 + i);
    }
    const bool live = valid && (__float_as_uint(g1.w) & FL_ALIVE);
    Path p;
    p.alive = false;
    bool jobDone = false, needStart = false;
    unsigned nSamp = 0;
    // Groups are written back only when this segment changed them: sum (G4) at sample end; RAY_ENTER_LOCATION / DISTANCE_TRAVELED (G5) when the
    // transmission lobe won; incLight (G3) when it is not zero and not what memory holds.
    bool sampleDone = false, newJob = false, isProbe = false, incInMemory = false;
    float4 g3in = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint2 jobWords = make_uint2(0u, 0u);
    if (live) {
        unpackFlags(p, __float_as_uint(g1.w));
        // incLight of the running sample: +0.0 in every component unless the path has met an emitter and gone on (FL_INCNZ): only those lanes fetch it.
        // (directDiffuse parks its probe state in the group: that mode reads and writes it for every lane.)
        incInMemory = DIRECT || p.incNZ;
        if (!ONE_TRIP && !DIRECT && p.incNZ) g3 = ldS(st.G3 + i);
        if (TRANS) {
            // RAY_ENTER_LOCATION / DISTANCE_TRAVELED are read only while the path is inside a medium or owes an absorption term;
            // a transmission event on any other path fetches them late (shadeSegment), which is rare per lane but a round trip for its wave:
            // where the load rides in the batch below it costs none, and every live lane fetches them
            p.g5loaded = ONE_TRIP || p.inObj || p.applyAbs;
            if (!ONE_TRIP && p.g5loaded) g5 = ldS(st.G5 + i);
        }
        p.O = v3(g0.x, g0.y, g0.z); p.D = v3(g0.w, g1.x, g1.y); p.rng = __float_as_uint(g1.z);
        p.col = v3(g2.x, g2.y, g2.z);
        if (EARLY) {
            sampleDone = segmentEndsSample<FAST>(fc, p, h.x, __float_as_int(h.w));
            if (sampleDone) {
                if (!ONE_TRIP) g4 = ldS(st.G4 + i);
                nSamp = 1;
                if ((float)(p.sample + 1) < fc.SAMPLE_RES) needStart = true;      // loop condition :898
                else { jobDone = true; if (!ONE_TRIP) jobWords = st.J[i]; }
            }
            if (ONE_TRIP) {
                g3 = ldS(p.incNZ ? st.G3 + i : st.Z);
                if (TRANS) g5 = ldS(st.G5 + i);
                g4 = ldS(sampleDone ? st.G4 + i : st.Z);
                jobWords = *(jobDone ? st.J + i : reinterpret_cast<const uint2*>(st.Z));
            }
        }
        p.inc = (ONE_TRIP || incInMemory) ? v3(g3.x, g3.y, g3.z) : v3(0.0f);      // (ONE_TRIP: the zero block's +0.0)
        p.sum = v3(g4.x, g4.y, g4.z); p.pix = __float_as_uint(g4.w);      // (path tracing: of the lanes whose sample ends; the others neither read nor write them)
        p.fi = 0u; p.ls = 0u;                                       // the job's (frame slot, accumulator slot) wait in J until the job ends
        p.enter = v3(g5.x, g5.y, g5.z); p.dist = g5.w; p.g5dirty = false;
        if (!TRANS) p.g5loaded = true;
        g3in = make_float4(p.inc.x, p.inc.y, p.inc.z, 0.0f);
        if (STK == 8) { p.sc0 = __float_as_uint(s0.x); p.sc1 = __float_as_uint(s0.y); p.sc2 = __float_as_uint(s0.z); }
        else { p.sc0 = __float_as_uint(g2.w); p.sc1 = 0u; p.sc2 = 0u; }
        if (STK == 32) {
            p.sk[0] = __float_as_uint(s0.x); p.sk[1] = __float_as_uint(s0.y); p.sk[2] = __float_as_uint(s0.z); p.sk[3] = __float_as_uint(s0.w);
            p.sk[4] = __float_as_uint(s1.x); p.sk[5] = __float_as_uint(s1.y); p.sk[6] = __float_as_uint(s1.z); p.sk[7] = __float_as_uint(s1.w);
            p.sk[8] = __float_as_uint(s2.x); p.sk[9] = __float_as_uint(s2.y);
        }
        isProbe = DIRECT && p.probe;
        if (DIRECT) {
            sampleDone = directSegment<TEX>(sc, p, h.x, h.y, h.z, __float_as_int(h.w), st.HX, i);      // RAYTRACING == 0 (frag.glsl:911-912)
            if (sampleDone) {
                p.sum = p.sum + p.inc;                                 // col += trace(...)  (:910)
                p.sample++;
                nSamp = 1;
                if ((float)p.sample < fc.SAMPLE_RES) needStart = true;      // loop condition :898
                else { jobDone = true; jobWords = st.J[i]; }
            }
        }
    }
    // ---- 2. job pull: ballot + prefix count per wave, aggregated over the block's 4 waves through LDS, so the
    // scheduler word sees ONE atomic per 256 lanes per launch (a single address sustains only ~90 atomics/us)
    unsigned long long mask = __ballot(jobDone);
    if (lane == 0) sCntA[wave] = (unsigned)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < SHADE_BLOCK / 64; w++) total += sCntA[w];
        sBase = total ? (writeQueue ? jobEnd : atomicAdd(&ctl->nextJob, total)) : 0u;       // known dry: no need to ask
        if (total && sBase + total > jobEnd) ctl->exhausted[(iter + 1) & 3] = 1u;                      // an empty pull: the tail begins
    }
    __syncthreads();
    unsigned nextJob = 0u;
    bool gotJob = false;
    if (jobDone) {
        unsigned off = 0;
#pragma unroll
        for (int w = 0; w < SHADE_BLOCK / 64; w++) off += (w < wave) ? sCntA[w] : 0u;
        nextJob = sBase + off + (unsigned)__popcll(mask & ltMask);
        gotJob = nextJob < jobEnd;
    }
    // ---- 2b. tail of the batch: the slots that stay alive go into the next iteration's dense queue (one atomic per block)
    if (writeQueue) {
        const bool keep = live && p.alive && !(jobDone && !gotJob);
        unsigned long long mk = __ballot(keep);
        if (lane == 0) sCntB[wave] = (unsigned)__popcll(mk);
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned total = 0;
#pragma unroll
            for (int w = 0; w < SHADE_BLOCK / 64; w++) total += sCntB[w];
            sBase = total ? atomicAdd(&ctl->qCount[32 * ((iter + 1) & 1)], total) : 0u;
        }
        __syncthreads();
        if (keep) {
            unsigned off = 0;
#pragma unroll
            for (int w = 0; w < SHADE_BLOCK / 64; w++) off += (w < wave) ? sCntB[w] : 0u;
            qOut[sBase + off + (unsigned)__popcll(mk & ltMask)] = i;
        }
    }
    // ---- 3. the segment (frag.glsl:823-879), then what a finished sample / a finished job leaves behind
    LobePending L; L.N = v3(0.0f); L.Pcr = 0.0f; L.w = 0; L.needG = false;
    if (live && EARLY) {
        shadeSegment<STK, TEX, FAST>(sc, fc, p, h.x, h.y, h.z, __float_as_int(h.w), st.G5, st.HX, i, L);      // (its answer is sampleDone's)
        if (sampleDone) {
            p.sum = p.sum + p.inc;                                 // col += trace(...)  (:910)
            p.sample++;
            // the sample loop goes on in this job's stream: chooseRay's six draws, made before trace() ended the sample, are behind it
            if (!jobDone && L.needG) p.rng = skipSixDraws(p.rng);
        }
    }
    if (jobDone) {
        float sr = fc.SAMPLE_RES;
        stS(b.colbuf + (size_t)(jobWords.x % b.ringFrames) * b.nSlots + jobWords.y, make_float4(p.sum.x / sr, p.sum.y / sr, p.sum.z / sr, 1.0f));   // col /= SAMPLE_RES (:915)
        if (gotJob) { startJob(b, fc, nextJob, p); needStart = true; newJob = true; }
        else p.alive = false;
    }
    // ---- 4. ONE site of randLambertianDistVec: a lane whose path goes on draws the Gaussian vector of its lobe (chooseRay, :775-804), a lane that starts a
    // sample the one of its lens jitter (frag.glsl:899-908) — a lane is one or the other; every store stays in slot order
    const bool drawLobe = live && !sampleDone && L.needG;
    vec3 G = v3(0.0f);
    if (needStart || drawLobe) G = randLambertianDistVec<FAST>(p.rng);
    if (needStart) { tracePrologue<STK>(p); cameraRayFrom<FAST>(fc, b.W, b.H, (int)(p.pix & 0xffffu), (int)(p.pix >> 16), G, p.O, p.D); }
    else if (drawLobe) p.D = lobeDirection<FAST>(L.w, G, L.N, p.D, 0.0f, L.Pcr);
    if (live) {
        {   // incLight leaves zero only at an emitter whose sample goes on, and returns to it with the next sample (tracePrologue): most segments
            // neither read nor write the group
            const bool nz = (__float_as_uint(p.inc.x) | __float_as_uint(p.inc.y) | __float_as_uint(p.inc.z)) != 0u;
            const bool changed = __float_as_uint(p.inc.x) != __float_as_uint(g3in.x) || __float_as_uint(p.inc.y) != __float_as_uint(g3in.y) ||
                                 __float_as_uint(p.inc.z) != __float_as_uint(g3in.z);
            if (DIRECT) { if (changed) stS(st.G3 + i, make_float4(p.inc.x, p.inc.y, p.inc.z, 0.0f)); p.incNZ = false; }
            else { if (nz && (changed || !incInMemory)) stS(st.G3 + i, make_float4(p.inc.x, p.inc.y, p.inc.z, 0.0f)); p.incNZ = nz; }
        }
        stS(st.G0 + i, make_float4(p.O.x, p.O.y, p.O.z, p.D.x));
        stS(st.G1 + i, make_float4(p.D.y, p.D.z, __uint_as_float(p.rng), __uint_as_float(packFlags(p))));
        stS(st.G2 + i, make_float4(p.col.x, p.col.y, p.col.z, __uint_as_float(p.sc0)));
        if (sampleDone) stS(st.G4 + i, make_float4(p.sum.x, p.sum.y, p.sum.z, __uint_as_float(p.pix)));
        if (newJob) st.J[i] = make_uint2(p.fi, p.ls);
        if (STK == 8) stS(st.S0 + i, make_float4(__uint_as_float(p.sc0), __uint_as_float(p.sc1), __uint_as_float(p.sc2), 0.0f));
        if (STK == 32) storeStack32(st, i, p);
        if (TRANS) { if (p.g5dirty || newJob) stS(st.G5 + i, make_float4(p.enter.x, p.enter.y, p.enter.z, p.dist)); }
    }
    if (STATS) {                                  // statistics (count mode only): one atomic per wave
        unsigned long long lm = __ballot(live && !isProbe);      // a thickness probe is part of the same directDiffuse call
        unsigned long long sm = __ballot(nSamp != 0);
        if (lm && lane == (__ffsll((long long)lm) - 1)) atomicAdd(&ctl->cnt[PT_CNT_SEGMENTS], (unsigned long long)__popcll(lm));
        if (sm && lane == (__ffsll((long long)sm) - 1)) atomicAdd(&ctl->cnt[PT_CNT_SAMPLES], (unsigned long long)__popcll(sm));
    }
}

// ---- the steps the accumulate kernels share, each stated once
// the pixel of accumulator slot ls: a whole image's slot is its pixel, a shard's follows its pixel list; false: no pixel of the shard lies there
__device__ __forceinline__ bool slotPixel(const Batch& b, unsigned ls, int& gp) {
    if (b.shardCount == 1) { gp = (int)ls; return true; }
    if (ls >= (unsigned)b.nLocal) return false;
    gp = b.pixList[ls];
    return true;
}
// the colour row of stream frame f at colbuf slot `slot`
__device__ __forceinline__ float4 frameColour(const Batch& b, unsigned f, unsigned slot) { return ldS(b.colbuf + (size_t)(f % b.ringFrames) * b.nSlots + slot); }
// the FRAME rule of frag.glsl:924-933: the frame numbered 1 restarts the image, every other one is added to it and counted
__device__ __forceinline__ bool restartsImage(int frameCount) { return (float)frameCount == 1.0f; }
__device__ __forceinline__ float4 frameRestart(float4 c) { return make_float4(c.x, c.y, c.z, 1.0f); }
__device__ __forceinline__ float4 frameAdd(float4 F, float4 c) { return make_float4(F.x + c.x, F.y + c.y, F.z + c.z, F.w + 1.0f); }
__device__ __forceinline__ float4 frameRule(float4 F, float4 c, int frameCount) { return restartsImage(frameCount) ? frameRestart(c) : frameAdd(F, c); }
// the luminance of a frame's colour (include/pt_adaptive.h; the parentheses are the order of the float32 sum) and T += (Y, Y*Y, 1, 0)
__device__ __forceinline__ float luminance(float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
__device__ __forceinline__ float4 momentsAdd(float4 T, float Y) { return make_float4(T.x + Y, T.y + Y * Y, T.z + 1.0f, 0.0f); }

// FRAME accumulation, frag.glsl:924-933, over one batch's frames in u_frameCount order (stream frames f0 .. f0+nFrames-1)
__global__ void __launch_bounds__(BLOCK) k_accumulate(Batch b, const FrameConst* fcp, float4* frame, unsigned f0, int nFrames, int firstFrame) {
    unsigned ls = blockIdx.x * BLOCK + threadIdx.x;
    if (ls >= (unsigned)b.nSlots) return;
    int gp;
    if (!slotPixel(b, ls, gp)) return;
    const FrameConst& fc = *fcp;
    if (inMouseOverlay(fc, gp % b.W, gp / b.W)) return;
    float4 F = frame[ls];
    for (int f = 0; f < nFrames; f++) F = frameRule(F, frameColour(b, f0 + (unsigned)f, ls), firstFrame + f);
    frame[ls] = F;
}

// k_accumulate with the luminance moments of include/pt_guided.h: the same slots, overlay and FRAME arithmetic, and T += (Y, Y*Y, 1, 0) per frame in
// u_frameCount order (k_accumulate_adaptive's update), restarted with FRAME by a frame numbered 1
__global__ void __launch_bounds__(BLOCK) k_accumulate_moments(Batch b, const FrameConst* fcp, float4* frame, float4* stats, unsigned f0, int nFrames, int firstFrame) {
    unsigned ls = blockIdx.x * BLOCK + threadIdx.x;
    if (ls >= (unsigned)b.nSlots) return;
    int gp;
    if (!slotPixel(b, ls, gp)) return;
    const FrameConst& fc = *fcp;
    if (inMouseOverlay(fc, gp % b.W, gp / b.W)) return;
    float4 F = frame[ls], T = stats[ls];
    for (int f = 0; f < nFrames; f++) {
        const float4 c = frameColour(b, f0 + (unsigned)f, ls);
        const float Y = luminance(c);
        if (restartsImage(firstFrame + f)) { F = frameRestart(c); T = make_float4(Y, Y * Y, 1.0f, 0.0f); }      // one branch: T restarts with FRAME
        else { F = frameAdd(F, c); T = momentsAdd(T, Y); }
    }
    frame[ls] = F;
    stats[ls] = T;
}

// DEBUG != 0 (frag.glsl:916-918): the traversal heat-map of debugRayScene (:539-547) — no random numbers, no samples.  One thread per
// local pixel; every BVH is traversed on its own from closest_t = 1e30 with the un-offset ORIGIN and the un-normalised primary
// direction (exactly the thickness probe's rayBVH call), and rayBVH's .col (:534) is rebuilt from the traversal counters:
// boxTests = 2 per inner node popped, 0.1 per leaf popped, triTests never incremented.  The frames of the batch add the same colour.
__global__ void __launch_bounds__(64) k_debug_heatmap(DevScene sc, Batch b, const FrameConst* fcp, float4* frame, int firstFrame, int nFrames) {
    __shared__ int stk[64 * 64];
    unsigned ls = blockIdx.x * 64 + threadIdx.x;
    if (ls >= (unsigned)b.nLocal) return;
    const FrameConst& fc = *fcp;
    const unsigned xy = b.pixXY[ls];
    const int px = (int)(xy & 0xffffu), py = (int)(xy >> 16);
    uint32_t index;
    if (!pixelIndex(fc, b.W, b.H, px, py, index) || inMouseOverlay(fc, px, py)) return;
    float tcx = ((float)px + 0.5f) / (float)b.W, tcy = ((float)py + 0.5f) / (float)b.H;
    vec3 q = v3(((tcx * 2.0f - 1.0f) * -1.0f) * fc.screenSize, ((tcy * 2.0f - 1.0f) * fc.screenHratio) * fc.screenSize, fc.focalLength);
    const vec3 direction = vecmat(q, fc.camRot);                   // :894, not normalised
    const vec3 ORIGIN = v3(fc.origin[0], fc.origin[1], fc.origin[2]);
    vec3 ret = v3(0.0f);
    for (int ob = 0; ob < sc.numObj; ob++) {
        Counters c;
        float t, u, v; int prim;
        intersectScene<true>(sc, ORIGIN, direction, stk + threadIdx.x, 64, nullptr, nullptr, t, u, v, prim, c, true, ob);
        const int boxTests = (int)c.boxtests - 1;                  // without the root test of :468
        const int leaves = (int)c.nodes - boxTests / 2;
        float ocx = 0.0f;
        for (int k = 0; k < leaves; k++) ocx = ocx + 0.1f;
        const float cx = ocx * 0.1f + 0.0f + exp_(0.02f * (float)(0 - 150)), cz = 0.0f * 0.1f + exp_(0.01f * (float)(boxTests - 200)) + 0.0f;
        ret = ret + v3(cx / (float)sc.numObj, 0.0f / (float)sc.numObj, cz / (float)sc.numObj);
    }
    const unsigned slot = (b.shardCount == 1) ? (unsigned)(py * b.W + px) : ls;
    float4 F = frame[slot];
    for (int f = 0; f < nFrames; f++) {
        F = frameRule(F, make_float4(ret.x, ret.y, ret.z, 0.0f), firstFrame + f);
    }
    frame[slot] = F;
}

// Which of the (up to 8) oldest batches that have not been accumulated yet does a live slot still work on?  ends.f[k] = first stream frame BEHIND the k-th of
// them (ascending): a live slot on frame f keeps the first batch with f < ends.f[k] busy.  One pass over the flags per host poll.
struct ScanEnds { unsigned f[8]; int n; };
// The host's look at the scheduler words: ONE wave copies Control into the group's snapshot in pinned, coherent host memory and, behind a system-scope fence, writes
// the group's number into the group's stamp.  The host reads both without a runtime call (no event, no copy engine, no synchronisation of the stream): this is the form
// that was verified under the checking allocator while a host heap corruption was being traced (profiles/r06_f_runtime_write_after_free.txt; its cause turned out to be
// the destruction of a stream, see takeStream in pt_stream_dev.hpp).
__global__ void __launch_bounds__(64) k_snapshot(const Control* ctl, Control* snap, volatile unsigned* stamp, unsigned seq) {
    const unsigned* s = reinterpret_cast<const unsigned*>(ctl);
    unsigned* d = reinterpret_cast<unsigned*>(snap);
    for (unsigned i = threadIdx.x; i < sizeof(Control) / 4; i += 64) d[i] = s[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) { *stamp = seq; __threadfence_system(); }
}
__global__ void __launch_bounds__(BLOCK) k_scan_inflight(State st, int nSlots, ScanEnds ends, Control* ctl) {
    unsigned i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (unsigned)nSlots) return;
    if (!(__float_as_uint(st.G1[i].w) & FL_ALIVE)) return;
    const unsigned f = st.J[i].x;
    if (f >= ends.f[ends.n - 1]) return;
    int k = 0;
    while (f >= ends.f[k]) k++;
    ctl->busy[k] = 1u;
}

// fragColor -> UNORM8 framebuffer -> glReadPixels(GL_RGB) -> Java signed-byte packing -> vertical flip (dispatch.java:804-833)
// PER_PIXEL (pt_read_display_mean, adaptive images): every pixel divided by its own count F.w; a count of 0 gives 0/0 = NaN, which the clamp shows as 0
template <bool PER_PIXEL>
__global__ void __launch_bounds__(BLOCK) k_display(const float4* frame, int W, int H, float frameCount, int javaBytes, unsigned char* out) {
    int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= W * H) return;
    int x = i % W, y = i / W;
    float4 F = frame[i];
    if (PER_PIXEL) frameCount = F.w;
    float v[3] = {F.x / frameCount, F.y / frameCount, F.z / frameCount};
    int q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float t = (v[k] != v[k]) ? 0.0f : (v[k] < 0.0f ? 0.0f : (v[k] > 1.0f ? 1.0f : v[k]));
        q[k] = (int)__builtin_floorf(t * 255.0f + 0.5f);
    }
    int r = q[0], g = q[1], b = q[2];
    if (javaBytes) {
        int pix = (int)((unsigned)(int)(signed char)r << 16) + (int)((unsigned)(int)(signed char)g << 8) + (int)(signed char)b;
        r = (pix >> 16) & 0xff; g = (pix >> 8) & 0xff; b = pix & 0xff;
    }
    unsigned char* o = out + 3 * ((size_t)(H - 1 - y) * W + x);
    o[0] = (unsigned char)r; o[1] = (unsigned char)g; o[2] = (unsigned char)b;
}

// ---- first-hit feature records (include/pt_denoise.h).  One ray per pixel of the whole image, slot = y*W + x: main()'s camera ray with the lens offset
// zero (cameraRayFrom, G = 0), as a live path-state record of an intersect launch; lanes beyond the image are dead records.
__global__ void __launch_bounds__(BLOCK) k_feature_rays(const FrameConst* fcp, int W, int H, State st, int nSlots) {
    const unsigned i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (unsigned)nSlots) return;
    if (i >= (unsigned)(W * H)) { st.G0[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); st.G1[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); return; }
    vec3 O, D;
    cameraRayFrom(*fcp, W, H, (int)(i % (unsigned)W), (int)(i / (unsigned)W), v3(0.0f), O, D);
    st.G0[i] = make_float4(O.x, O.y, O.z, D.x);
    st.G1[i] = make_float4(D.y, D.z, 0.0f, __uint_as_float(FL_ALIVE));
    st.H[i] = make_float4(1e30f, 0.0f, 0.0f, __int_as_float(PRIM_NONE));
}
// The 64-B record of each pixel from its ray and hit record (and the side record HX of an ellipsoid hit): what trace() decodes at :823-830
__global__ void __launch_bounds__(BLOCK) k_feature_record(DevScene sc, State st, int n, float4* feat) {
    const unsigned i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (unsigned)n) return;
    const float4 g0 = st.G0[i], g1 = st.G1[i], h = st.H[i];
    const vec3 O = v3(g0.x, g0.y, g0.z), D = v3(g0.w, g1.x, g1.y);
    const int prim = __float_as_int(h.w);
    float4 f0 = make_float4(-1.0f, 0.0f, 0.0f, 0.0f), f1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1)), f3 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int mat = -1;
    if (segmentHit(h.x, prim)) {                                   // rayScene's result.distance is -1 on a miss (:651)
        vec3 loc, N;
        surfaceAt(sc, O, D, h.x, h.y, h.z, prim, loc, N, mat);
        MatRec m = sc.mats[mat];
        float uvx, uvy;
        uvOfHit(sc, prim, h.y, h.z, st.HX, i, uvx, uvy);
        if (m.hasMaps) applyMaps(sc, m, uvx, uvy, N);
        const int code = (prim & PRIM_ELLIPSOID) ? 3 * 0x1000000 + (prim & 0xffffff) : 0x1000000 + prim;     // hit.type * 0x1000000 + hit.id
        f0 = make_float4(h.x, N.x, N.y, N.z);
        f1 = make_float4(m.Kd[0], m.Kd[1], m.Kd[2], __int_as_float(code));
        f3 = make_float4(uvx, uvy, 0.0f, 0.0f);
    }
    float4* r = feat + 4 * (size_t)i;
    r[0] = f0; r[1] = f1; r[2] = make_float4(D.x, D.y, D.z, __int_as_float(mat)); r[3] = f3;
}

// ---- seen-through feature records (include/pt_through.h).  One launch per link of the chain, behind the intersect launch of the same probe pool:
// steps 2-8 of the header for every live lane.  The lane writes the record of the surface it found (and the segment that found it, the parity
// probe's `rays`) and either its next ray into G0 / G1 with H reset, as k_feature_rays writes one, or a dead record.  The chain state between the
// launches lives in X, planes of `plane` float4: X0 = (tint.rgb, L), X1 = (k | stack size << 8, first-hit material, sc0, sc1), X2 = (sc2, 0, 0, 0)
// with 8-bit index-stack codes; STK == 32: X2, X3, X4 = the ten floats of the stack.  Exact numeric contract throughout.
struct ThroughRule { int maxDepth; float minWeight; int lobes, flags; };
PM_DEV bool finiteF(float x) { return __builtin_fabsf(x) <= 3.4028235e38f; }      // false for NaN and the infinities
template <int STK>
__global__ void __launch_bounds__(BLOCK) k_through_step(DevScene sc, State st, int n, ThroughRule rule, int step, float4* X, unsigned plane, float4* feat,
                                                        float4* rays) {
    const unsigned i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (unsigned)n) return;
    const float4 g0 = st.G0[i], g1 = st.G1[i];
    if (!(__float_as_uint(g1.w) & FL_ALIVE)) return;
    const float4 h = st.H[i];
    const vec3 O = v3(g0.x, g0.y, g0.z), D = v3(g0.w, g1.x, g1.y);
    const int prim = __float_as_int(h.w);
    float4* r = feat + 4 * (size_t)i;
    float4* ry = rays + 2 * (size_t)i;
    const float4 dead = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    Path p;
    p.sc0 = p.sc1 = p.sc2 = 0u;
#pragma unroll
    for (int s = 0; s < 10; s++) p.sk[s] = 0u;
    vec3 tint = v3(1.0f);
    float L = 0.0f;
    int k = 0, firstMat = -1;
    if (step == 0) {                                              // trace()'s prologue (:816): {1.0029}
        p.stackSize = 0;
        if (STK) addToIndiceStack<STK>(p, stackElemAir<STK>()); else p.stackSize = 1;
    } else {
        const float4 x0 = X[i], x1 = X[plane + i];
        tint = v3(x0.x, x0.y, x0.z); L = x0.w;
        const unsigned ks = __float_as_uint(x1.x);
        k = (int)(ks & 0xffu); p.stackSize = (int)(ks >> 8);
        firstMat = __float_as_int(x1.y);
        p.sc0 = __float_as_uint(x1.z); p.sc1 = __float_as_uint(x1.w);
        if (STK == 8) p.sc2 = __float_as_uint(X[2 * (size_t)plane + i].x);
        if (STK == 32) {
            const float4 a = X[2 * (size_t)plane + i], b = X[3 * (size_t)plane + i], c = X[4 * (size_t)plane + i];
            p.sk[0] = __float_as_uint(a.x); p.sk[1] = __float_as_uint(a.y); p.sk[2] = __float_as_uint(a.z); p.sk[3] = __float_as_uint(a.w);
            p.sk[4] = __float_as_uint(b.x); p.sk[5] = __float_as_uint(b.y); p.sk[6] = __float_as_uint(b.z); p.sk[7] = __float_as_uint(b.w);
            p.sk[8] = __float_as_uint(c.x); p.sk[9] = __float_as_uint(c.y);
        }
    }
    if (!segmentHit(h.x, prim)) {                                  // step 1: the record written last stays; a first ray that misses gets k_feature_record's
        if (step == 0) {
            r[0] = make_float4(-1.0f, 0.0f, 0.0f, 0.0f); r[1] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
            r[2] = make_float4(D.x, D.y, D.z, __int_as_float(-1)); r[3] = dead;
            ry[0] = make_float4(O.x, O.y, O.z, -1.0f); ry[1] = make_float4(D.x, D.y, D.z, __int_as_float(0));
        }
        st.G1[i] = dead;
        return;
    }
    // step 2 (frag.glsl:823-830)
    vec3 loc, N; int mat;
    surfaceAt(sc, O, D, h.x, h.y, h.z, prim, loc, N, mat);
    MatRec m = sc.mats[mat];
    float uvx, uvy;
    uvOfHit(sc, prim, h.y, h.z, st.HX, i, uvx, uvy);
    if (m.hasMaps) applyMaps(sc, m, uvx, uvy, N);
    L = L + h.x;
    // step 3
    const int code = (prim & PRIM_ELLIPSOID) ? 3 * 0x1000000 + (prim & 0xffffff) : 0x1000000 + prim;
    const vec3 Kd = v3(m.Kd[0], m.Kd[1], m.Kd[2]);
    const vec3 through = tint * Kd;
    if (k == 0) firstMat = mat;
    const int word = (k == 0 || !(rule.flags & 1)) ? mat : (int)(((unsigned)k << 24) | ((unsigned)firstMat << 12) | (unsigned)mat);
    const float4 d0 = step == 0 ? make_float4(D.x, D.y, D.z, 0.0f) : r[2];
    r[0] = make_float4(L, N.x, N.y, N.z);
    r[1] = make_float4(through.x, through.y, through.z, __int_as_float(code));
    r[2] = make_float4(d0.x, d0.y, d0.z, __int_as_float(word));
    r[3] = make_float4(uvx, uvy, __int_as_float(k), 0.0f);
    ry[0] = make_float4(O.x, O.y, O.z, h.x); ry[1] = make_float4(D.x, D.y, D.z, __int_as_float(k));
    if (k >= rule.maxDepth) { st.G1[i] = dead; return; }          // step 4
    // the rest of step 2 (:830-840)
    const float ND = dot(N, D);
    const vec3 Nf = N * (ND > 0.0f ? -1.0f : 1.0f);
    float n1 = 1.0f, n2 = 1.0f;
    if (STK) {                                                    // as shadeSegment restates :833-840, stale slot and full stack included
        const float s0 = indiceStackSlot<STK>(sc, p, 0), s1 = indiceStackSlot<STK>(sc, p, 1);
        if (ND < 0.0f) { const bool full = p.stackSize >= 10; n1 = (full || p.stackSize == 0) ? s1 : s0; n2 = full ? s0 : m.Ni; addToIndiceStack<STK>(p, stackElemOf<STK>(m)); }
        else { n1 = s0; n2 = s1; removeFirstOfIndiceStack<STK>(p); }
    }
    // step 5: chooseRay's weights (:745-765), as chooseLobe computes them under the exact contract
    float reflectionWeight = 1.0f - m.Pr;
    const float clearcoatWeight = m.Pc;
    float transmissionWeight = (m.Tr > 0.0f ? m.Tr : (m.Tf[0] > 0.0f ? (m.Tf[0] + m.Tf[1] + m.Tf[2]) / 3.0f : 0.0f));
    float fresnel = 0.0f;
    if (m.illum == 5 || m.illum == 7 || transmissionWeight > 0.0f) {
        fresnel = fresnelReflectAmount<false>(n1, n2, Nf, D);
        reflectionWeight += fresnel * m.Pr;
        transmissionWeight *= (1.0f - fresnel);
    }
    const float diffuseWeight = (1.0f - m.Pm) * (1.0f - transmissionWeight) * (1.0f - fresnel);
    const float totalWeight = diffuseWeight + reflectionWeight + clearcoatWeight + transmissionWeight;
    reflectionWeight /= totalWeight; transmissionWeight /= totalWeight;
    // steps 6 and 7
    vec3 nd;
    if ((rule.lobes & 1) && reflectionWeight >= rule.minWeight && reflectionWeight >= transmissionWeight) nd = reflect(D, Nf);
    else if ((rule.lobes & 2) && transmissionWeight >= rule.minWeight) nd = refractT<false>(D, Nf, n1 / n2);
    else { st.G1[i] = dead; return; }
    if (!(finiteF(nd.x) && finiteF(nd.y) && finiteF(nd.z)) || (nd.x == 0.0f && nd.y == 0.0f && nd.z == 0.0f)) { st.G1[i] = dead; return; }
    // step 8
    k++;
    st.G0[i] = make_float4(loc.x, loc.y, loc.z, nd.x);
    st.G1[i] = make_float4(nd.y, nd.z, 0.0f, __uint_as_float(FL_ALIVE));
    st.H[i] = make_float4(1e30f, 0.0f, 0.0f, __int_as_float(PRIM_NONE));
    X[i] = make_float4(through.x, through.y, through.z, L);
    X[plane + i] = make_float4(__uint_as_float((unsigned)k | ((unsigned)p.stackSize << 8)), __int_as_float(firstMat), __uint_as_float(p.sc0), __uint_as_float(p.sc1));
    if (STK == 8) X[2 * (size_t)plane + i] = make_float4(__uint_as_float(p.sc2), 0.0f, 0.0f, 0.0f);
    if (STK == 32) {
        X[2 * (size_t)plane + i] = make_float4(__uint_as_float(p.sk[0]), __uint_as_float(p.sk[1]), __uint_as_float(p.sk[2]), __uint_as_float(p.sk[3]));
        X[3 * (size_t)plane + i] = make_float4(__uint_as_float(p.sk[4]), __uint_as_float(p.sk[5]), __uint_as_float(p.sk[6]), __uint_as_float(p.sk[7]));
        X[4 * (size_t)plane + i] = make_float4(__uint_as_float(p.sk[8]), __uint_as_float(p.sk[9]), 0.0f, 0.0f);
    }
}

// ---- adaptive sampling (include/pt_adaptive.h).  The selection rule over the per-slot statistics T = (sY, sYY, n, 0), in the order the header states it
// (float32, no contraction: the build's -ffp-contract=off, IEEE divides).  NaN anywhere: every comparison false, the pixel stays inactive.
struct AdaptRule { float relErr, absErr, mouseX, mouseY, resolution; int minFrames, maxFrames; };
// the rule's mouse fields as the frame constants inMouseOverlay reads
__device__ __forceinline__ bool underOverlay(const AdaptRule& r, int px, int py) {
    FrameConst fc{};
    fc.mouse[0] = r.mouseX; fc.mouse[1] = r.mouseY; fc.resolution = r.resolution;
    return inMouseOverlay(fc, px, py);
}
__device__ __forceinline__ bool adaptiveActive(const AdaptRule& r, float4 T, int px, int py) {
    if (underOverlay(r, px, py)) return false;
    const float n = T.z;
    if (r.maxFrames > 0 && n >= (float)r.maxFrames) return false;
    if (n < (float)r.minFrames) return true;
    const float mean = T.x / n;
    const float var = (T.y - T.x * mean) / (n - 1.0f);
    const float err2 = var / n;
    const float tol = fmaxf(r.relErr * fabsf(mean), r.absErr);
    return err2 > tol * tol;
}
// Stable compaction of the active pixels of the job-order list pixXY, in three passes: (1) the rule per pixel, a flag byte and the block's count
// (wave64 ballot / popcount), (2) one block turns the counts into exclusive block offsets and the total, (3) every active pixel writes its entry at
// block offset + the active pixels before it in its block.  The order is the list's: deterministic, and the tiles stay together.
__global__ void __launch_bounds__(BLOCK) k_adaptive_select(const unsigned* pixXY, int nLocal, int W, int shardCount, const float4* stats, AdaptRule r,
                                                           unsigned char* flag, unsigned* blkCount) {
    __shared__ unsigned sCnt[BLOCK / 64];
    const unsigned k = blockIdx.x * BLOCK + threadIdx.x;
    bool on = false;
    if (k < (unsigned)nLocal) {
        const unsigned xy = pixXY[k];
        const int px = (int)(xy & 0xffffu), py = (int)(xy >> 16);
        const unsigned slot = shardCount == 1 ? (unsigned)(py * W + px) : k;
        on = adaptiveActive(r, stats[slot], px, py);
        flag[k] = on ? 1 : 0;
    }
    const unsigned long long mask = __ballot(on);
    if ((threadIdx.x & 63) == 0) sCnt[threadIdx.x >> 6] = (unsigned)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; w++) t += sCnt[w];
        blkCount[blockIdx.x] = t;
    }
}
// k_adaptive_select's output contract for a given selection (include/pt_steer.h, pt_render_mask): entry k of the job-order list is active iff
// mask[py*W + px] != 0 (the whole image's W*H bytes, FRAME order) and it is not under the overlay (r's mouse fields; the rule fields unused)
__global__ void __launch_bounds__(BLOCK) k_adaptive_select_mask(const unsigned* pixXY, int nLocal, int W, const unsigned char* mask, AdaptRule r,
                                                                unsigned char* flag, unsigned* blkCount) {
    __shared__ unsigned sCnt[BLOCK / 64];
    const unsigned k = blockIdx.x * BLOCK + threadIdx.x;
    bool on = false;
    if (k < (unsigned)nLocal) {
        const unsigned xy = pixXY[k];
        const int px = (int)(xy & 0xffffu), py = (int)(xy >> 16);
        on = mask[(size_t)py * W + px] != 0 && !underOverlay(r, px, py);
        flag[k] = on ? 1 : 0;
    }
    const unsigned long long m = __ballot(on);
    if ((threadIdx.x & 63) == 0) sCnt[threadIdx.x >> 6] = (unsigned)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; w++) t += sCnt[w];
        blkCount[blockIdx.x] = t;
    }
}
// include/pt_fill.h's lattice as k_adaptive_select_mask's input: mask[y*W + x] = (x % stride == phaseX && y % stride == phaseY), W*H bytes
__global__ void __launch_bounds__(BLOCK) k_lattice_mask(unsigned char* mask, int W, int n, int stride, int phaseX, int phaseY) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int y = i / W, x = i - y * W;
    mask[i] = (x % stride == phaseX && y % stride == phaseY) ? 1 : 0;
}
// one block of BLOCK threads: blk[0..nb) counts -> exclusive offsets in place, *total = their sum
__global__ void __launch_bounds__(BLOCK) k_adaptive_scan(unsigned* blk, int nb, unsigned* total) {
    __shared__ unsigned sv[BLOCK];
    unsigned carry = 0;
    for (int base = 0; base < nb; base += BLOCK) {
        const int i = base + (int)threadIdx.x;
        const unsigned v = i < nb ? blk[i] : 0u;
        sv[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < BLOCK; d <<= 1) {                     // inclusive Hillis-Steele scan
            const unsigned a = threadIdx.x >= (unsigned)d ? sv[threadIdx.x - d] : 0u;
            __syncthreads();
            sv[threadIdx.x] += a;
            __syncthreads();
        }
        if (i < nb) blk[i] = carry + sv[threadIdx.x] - v;
        carry += sv[BLOCK - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}
// outXY: the stream's pixXY; outSlot (shards only): the accumulator slot of every entry
__global__ void __launch_bounds__(BLOCK) k_adaptive_compact(const unsigned* pixXY, int nLocal, const unsigned char* flag, const unsigned* blkOff,
                                                            unsigned* outXY, int* outSlot) {
    __shared__ unsigned sCnt[BLOCK / 64];
    const unsigned k = blockIdx.x * BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool on = k < (unsigned)nLocal && flag[k] != 0;
    const unsigned long long mask = __ballot(on);
    if (lane == 0) sCnt[wave] = (unsigned)__popcll(mask);
    __syncthreads();
    if (!on) return;
    unsigned off = blkOff[blockIdx.x];
#pragma unroll
    for (int w = 0; w < BLOCK / 64; w++) off += (w < wave) ? sCnt[w] : 0u;
    off += (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
    outXY[off] = pixXY[k];
    if (outSlot) outSlot[off] = (int)k;
}
// FRAME accumulation of an adaptive batch (k_accumulate's rule, frag.glsl:924-933) over the active list, and the statistics, both in u_frameCount order.
// The list entry i is the stream's pixel i: its frame rows sit at colbuf slot py*W+px (one shard) or i (shards: startJob's ls = k); its accumulator
// slot is py*W+px or b.pixList[i] (an adaptive stream's pixList holds the entries' slots).  Mouse-overlay pixels are never on the list.
__global__ void __launch_bounds__(BLOCK) k_accumulate_adaptive(Batch b, float4* frame, float4* stats, unsigned f0, int nFrames, int firstFrame) {
    const unsigned i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (unsigned)b.nLocal) return;
    const unsigned xy = b.pixXY[i];
    const unsigned slot = b.shardCount == 1 ? (xy >> 16) * (unsigned)b.W + (xy & 0xffffu) : (unsigned)b.pixList[i];
    const unsigned cs = b.shardCount == 1 ? slot : i;
    float4 F = frame[slot], T = stats[slot];
    for (int f = 0; f < nFrames; f++) {
        const float4 c = frameColour(b, f0 + (unsigned)f, cs);
        F = frameRule(F, c, firstFrame + f);
        T = momentsAdd(T, luminance(c));                          // not restarted by a frame numbered 1, unlike k_accumulate_moments
    }
    frame[slot] = F;
    stats[slot] = T;
}

__global__ void k_unshard(const float4* gathered, const int* maps, int nSlots, int shardCount, float4* full) {
    size_t k = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= (size_t)nSlots * shardCount) return;
    int gp = maps[k];
    if (gp >= 0) full[gp] = gathered[k];
}

__global__ void k_init_control(Control* ctl) {                     // a new frame stream: job ids restart at 0
    ctl->nextJob = 0; ctl->jobEnd = 0; ctl->needRevive = 1; ctl->oldestBusy = 0; for (int k = 0; k < 8; k++) ctl->busy[k] = 0;
    for (int k = 0; k < 4; k++) ctl->exhausted[k] = 0;
    ctl->qCount[0] = 0; ctl->qCount[32] = 0;
}
// addJobs more jobs for the running stream.  If the pool already ran dry (a pull came back empty), the ids it overshot by
// were never started: hand them out again and let dead slots pull (k_revive); the tail queue is dropped, every slot is visited.
__global__ void k_submit(Control* ctl, unsigned addJobs, int streamStart, unsigned nSlots) {
    bool dry = false;
    for (int k = 0; k < 4; k++) { dry = dry || ctl->exhausted[k] != 0; ctl->exhausted[k] = 0; }
    if (ctl->nextJob > ctl->jobEnd) { ctl->nextJob = ctl->jobEnd; dry = true; }
    ctl->jobEnd += addJobs;
    ctl->needRevive = (dry || streamStart == 2) ? 1u : 0u;                              // 2: the pool has just grown by dead slots
    if (streamStart == 1) { ctl->needRevive = 2u; ctl->nextJob = min(nSlots, addJobs); }      // fresh pool: slot i starts job i, no pulling
    ctl->qCount[0] = 0; ctl->qCount[32] = 0;
}

__global__ void k_debug_math(int fn, const float* x, const float* y, float* out, size_t n) {
    size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    float r;
    switch (fn) {
        case 0: r = sin_(x[i]); break;
        case 1: r = cos_(x[i]); break;
        case 2: r = log_(x[i]); break;
        case 3: r = exp_(x[i]); break;
        case 4: r = atan2_(x[i], y[i]); break;
        case 5: r = asin_(x[i]); break;
        // the RNG of frag.glsl:686-694 on the device (K1 vectors): x carries the uint32 state as bits
        case 6: { uint32_t st = __float_as_uint(x[i]); NextRandom(st); r = __uint_as_float(st); break; }                     // state after one call
        case 7: { uint32_t st = __float_as_uint(x[i]); r = __uint_as_float(NextRandom(st)); break; }                         // result of that call
        case 8: { uint32_t st = __float_as_uint(x[i]); r = random_(st); break; }                                             // random()
        case 9: r = unorm8((uint32_t)x[i]); break;                                                                           // byte / 255.0f as the samplers evaluate it
        default: r = __builtin_nanf("");
    }
    out[i] = r;
}
