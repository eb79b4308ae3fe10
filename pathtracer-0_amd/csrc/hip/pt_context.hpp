// pt_context.hpp — a render context and what it owns (included by pt_hip.hip behind pt_kernels.hpp, whose State, Control and Batch it holds; not a
// translation unit): the error text of the calling thread, struct pt_ctx, the upload of the scene that pt_scene_layout.hpp
// laid out, the path pool, the frame inputs current at a call, and a context's accumulator slots to and from a whole host image.  Nothing here
// launches a render kernel: that is pt_stream_dev.hpp.
namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
int fail(const ptp::Refused& r) { return r.code ? fail(r.code, r.msg) : 0; }      // a refusal of the image history (pt_image_history.hpp), or 0
#define HIP_TRY(x)                                                                                         \
    do {                                                                                                   \
        hipError_t e_ = (x);                                                                               \
        if (e_ != hipSuccess) return fail(PT_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));    \
    } while (0)

}  // namespace

struct MultiCtx;
struct pt_pose;
struct pt_ctx;
namespace {
int settleScene(pt_ctx* c);                                   // pt_pose_host.hpp
int settledScene(pt_ctx* c, SceneBuffers** b);                // below
size_t hostTriangleCount(const pt_ctx* c);                    // below

// A context's host copies of the bindings and textures.  Bindings 3 and 10 (tris, bvhdata) may be BEHIND a pose (include/pt_pose.h): the posed
// binding 3 and the refit binding 10 then lie in the pose's plan on the device.  So those two members, and the buffers as a whole, are reachable
// through ONE path only, settledScene(), which brings them up to date first; every other member is read and written directly.
class HostScene : private SceneBuffers {
  public:
    using SceneBuffers::origin; using SceneBuffers::rotation; using SceneBuffers::mouse; using SceneBuffers::params; using SceneBuffers::imp;
    using SceneBuffers::ellip; using SceneBuffers::mtl; using SceneBuffers::bvhtree; using SceneBuffers::leaftris; using SceneBuffers::objidx;
    using SceneBuffers::sky; using SceneBuffers::skyW; using SceneBuffers::skyH; using SceneBuffers::textures;
  private:
    friend int settleScene(pt_ctx* c);                        // the download itself
    friend int settledScene(pt_ctx* c, SceneBuffers** b);
    friend size_t hostTriangleCount(const pt_ctx* c);         // (a settle changes no length)
};

}  // namespace

struct pt_ctx {
    MultiCtx* multi = nullptr;      // != nullptr: a multi-GPU group (pt_create_multi, pt_multi.hpp); everything below then lives in its per-device contexts
    int device = 0, W = 0, H = 0, shardRank = 0, shardCount = 1;
    hipStream_t ownStream = nullptr, stream = nullptr;
    ptp::Options opt;               // what pt_set_option has stored (pt_options.hpp: the table there says what each member means)
    // spatial partition (opt.cuPartition) as built: the intersect launches on a stream whose CU mask holds that many eighths of every XCD's CUs, the shading
    // launches on the complement; events order extend(i) -> shade(i) -> extend(i+1), everything else stays on `stream`
    int cuPartitionBuilt = 0; hipStream_t sExt = nullptr, sShade = nullptr; hipEvent_t evExt = nullptr, evShade = nullptr, evHost = nullptr;
    HostScene buf;                  // raw SSBO contents and textures (host copies, glBufferData semantics): what layoutScene reads, through settledScene()
    // include/pt_pose.h: the poses created on this context, and the one whose plan holds the bindings 3 and 10 that the host copies are BEHIND
    // (nullptr: they are current)
    std::vector<pt_pose*> poses; pt_pose* behind = nullptr;
    Dev<uchar4> dTexels; Dev<TexRec> dTexTable;      // all textures beyond the sky in one allocation + the bindless-style table
    bool sceneDirty = true, frameInDirty = true;
    bool trans = false, anySubsurface = false, ambiguousTriObj = false, anyMaps = false; Dev<int> dTriObj;
    ptp::PlanScene built;           // the scene as built, as the launch planner reads it (buildScene): stack depth and entry width, record stride, eligibility, ...
    // device scene
    Dev<float4> dNodes, dTris, dShade; Dev<ObjRoot> dRoots; Dev<EllipRec> dEllip; Dev<MatRec> dMats;
    Dev<uchar4> dSky; Dev<float> dNiTable;
    int niBits = 0;                 // index-stack encoding of the path state: 0 no transmissive material (the stack is unobservable), 3 or 8 bits per slot, 32: the floats themselves
    Dev<unsigned char> dDisplay;      // scratch of pt_read_display (W*H*3 bytes, allocated on first use)
    DevScene sc{};
    // shard
    std::vector<int32_t> pixList; int nLocal = 0, nSlotsImg = 0; Dev<int> dPixList; Dev<unsigned> dPixXY; Dev<int> dAllMaps;
    static constexpr int IMAGES = ptp::ImageHistory::IMAGES;
    Dev<float4> dImage[IMAGES];     // FRAME images (more than one only after pt_next_image); hist.image() is the current one
    // path pool
    int allocSlots = 0; int allocNiBits = -1; bool allocHX = false;
    State st{};                     // the pool as the kernels take it; its groups are owned by dPool (in the order of ensurePool) and dPoolJ
    Dev<float4> dPool[9]; Dev<uint2> dPoolJ;
    Dev<float4> dZero;              // st.Z: zeroed when allocated (ensurePool), then read only; it outlives every pool
    Dev<unsigned> dQueue[2];        // dense slot queues of the batch tail, by iteration parity
    Dev<float4> dColbuf; Dev<int> dSeeds; int ringFrames = 0;      // per-frame rings of the stream (Batch)
    // frame-stream scheduler: its host view (pt_stream_sched.hpp), and what the device side of it needs
    ptp::StreamSched sched;
    Dev<FrameIn> dFrameIn; Dev<FrameConst> dFc; Dev<Control> dCtl;
    // per group in flight (StreamSched::grp, by slot): k_snapshot writes Control into the pinned snapshot and then the group's number into the pinned STAMP
    struct GroupPins { Pinned<Control, hipHostMallocCoherent> h; Pinned<volatile unsigned, hipHostMallocCoherent> stamp; } grp[2];
    Pinned<FrameIn> hFrameIn; Pinned<int32_t> hSeeds;   // pinned staging (hSeeds: ring like dSeeds)
    // stats, and what the hand-written intersect kernel needs
    bool timing = false;
    Dev<float> dNodes80;            // node records of the hand-written kernel: the two references + (min pair, max pair, min pair) per axis (80 B), or + pad + (min pair, max pair) (64 B)
    int asmGroupShift = 0;          // more than 8 BVHs: log2 of the objects per group box of the per-ray cull
    Dev<unsigned char> dAsmDbg;     // developer builds of the hand-written kernel (-DPT_ASM_DEBUG): its per-wave records
    std::string asmError;           // a failed load / launch of the hand-written kernel (surfaces as PT_ERR_HIP from the render call)
    uint64_t asmLaunches = 0;
    std::string asmWhyNot;          // why this scene cannot run on the hand-written kernel (built.asmEligible; pt_debug: reported by option 12)
    // per block size (256, 1024, 512 threads) six code objects: 16-bit stack entries, Packed18, the same two with v_rcp_f32 (relaxed contract), 24-bit entries exact / relaxed
    hipModule_t asmModule[18] = {}; hipFunction_t asmFn[18] = {}; std::string asmLoadError[18];
    int numCUs = 256;
    int streamsOnDevice = 1;        // streams of the same multi-stream context on this context's GPU (pt_create_multi)
    bool streamFast = false;        // the relaxed numeric contract (opt.fastContract) as the running stream was started with
    uint64_t hostCnt[PT_CNT_N] = {0};
    // adaptive sampling (include/pt_adaptive.h): per accumulator slot (sY, sYY, n, 0), allocated by the first pt_render_adaptive; the selection's scratch;
    // while adaptOn the running frame stream's pixel list is the active list (streamBatch), its nLocal adaptN
    Dev<float4> dStats; Dev<unsigned char> dAdaptFlag; Dev<unsigned> dAdaptBlk, dAdaptXY; Dev<int> dAdaptSlot;
    Pinned<unsigned> hAdaptCount; bool adaptOn = false; int adaptN = 0;
    // include/pt_steer.h: the whole image's selection mask (W*H bytes, pixel order), then, 4-byte aligned, k_gd_select's active count
    Dev<unsigned char> dSelMask;
    bool recordMoments = false;     // include/pt_guided.h: the frames of pt_render* also go into T (k_accumulate_moments) when they land in the current image
    // What the current image is a picture of (pt_image_history.hpp): the ring's camera records and the current image, the upload generations, the
    // validity of the mark and the hold, the keys of the record caches, whose frame constants are on the device.  The buffers below are what it describes
    ptp::ImageHistory hist;
    // The feature records (W*H x 4 float4) of one set of frame inputs, by ptp::RecordCache: first-hit records (include/pt_denoise.h), or seen-through
    // records with their last segments (`rays`, W*H x 2 float4; include/pt_through.h)
    struct Records { Dev<float4> recs, rays; } rec[ptp::RC_COUNT];
    Dev<float4> dDnCol[2], dDnGuide, dDnOut;      // the filters' colour ping-pong, packed guide (2 float4 per pixel) and output
    bool filteredThere = false;     // dDnOut holds the image of the last filter call (include/pt_bloom.h's PT_BLOOM_SRC_FILTERED): set and cleared where it is written
    Dev<float4> dBloomPyr, dBloomOut;      // include/pt_bloom.h: the pyramid (all levels in one allocation) and the composed image (W*H float4)
    // reprojection (include/pt_reproject.h): one flag byte per material (1 = view-dependent, buildScene); the scratch images, the kept counts
    // (two), the packed candidates of k_through_pack (W*H x 2 float4)
    Dev<unsigned char> dMatVD;
    Dev<float4> dRpFrame, dRpStats, dRpPack; Dev<unsigned> dRpKept;
    Dev<float4> dStatsWhole;        // a group's T gathered in pixel order on its first stream (reprojection, the guided filter)
    Dev<float4> dFill; Dev<unsigned> dFillCount;      // include/pt_fill.h: FRAME' (W*H float4) and k_gd_fill's count
    // include/pt_motion.h.  The mark: Rh (feat), the primitives' positions then on the device (3 float4 each) and on the host (9 floats per
    // triangle, 10 per ellipsoid); the positions now are packed per call into dMoveTri / dMoveEl
    struct Mark { int nTri = 0, nEl = 0; std::vector<float> tri, el; Dev<float4> feat, dTri, dEl; bool triOnDevice = false; } mark;      // triOnDevice: tri is still to be fetched from dTri
    Dev<float4> dMoveTri, dMoveEl;
    // include/pt_validate.h.  The hold (on a group's first stream): the held FRAME and T in pixel order (W*H float4 each); pt_history_merge's
    // kappa (W*H floats, only when asked for)
    struct Hold { Dev<float4> frame, stats; } hold;
    Dev<float> dKappa;
    struct KT { std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; size_t used = 0; int64_t launches = 0; double ms = 0; std::vector<float> each; } kt[4];
};

namespace {

// the pixels of a shard and their slots are pt_group_plan.hpp's (host only), in the kernels' tiles and blocks
static_assert(TILE_W == ptp::SHARD_TILE_W && TILE_H == ptp::SHARD_TILE_H && BLOCK == ptp::SHARD_BLOCK,
              "a shard's pixel list is dealt in the kernels' tiles, and its slots come in the blocks their launches cover");

// The scene build's device half: lays the buffers out on the host (layoutScene, pt_scene_layout.hpp), uploads the arrays, wires DevScene, and only then
// takes the layout's flags and modes into the context: a refused scene leaves the context as it was (sceneDirty stays set).
// THE access path to the host copies of bindings 3 and 10 and to the buffers as a whole: settles (settleScene, pt_pose_host.hpp: downloads what
// the two are behind by; nothing when they are current), then hands out the buffers
int settledScene(pt_ctx* c, SceneBuffers** b) {
    if (const int rc = settleScene(c)) return rc;
    *b = &c->buf;
    return 0;
}
size_t hostTriangleCount(const pt_ctx* c) { return c->buf.tris.size() / 40; }
void posesStale(pt_ctx* c);            // ... an accepted upload of binding 3 or 10-13, or a pt_move_geometry: the context's poses no longer describe it
void posesDestroy(pt_ctx* c);          // ... pt_destroy
// ... motionPack's triangle records (pt_motion_pack.hpp) of the posed binding 3 that on->behind holds, made on the device into `out` on on->stream:
// then == nullptr: the mark's own (flags 0); else flagged against the mark's records.  *nTri: the triangles
int poseMotionRecords(pt_ctx* on, const float4* then, int nThen, Dev<float4>& out, int* nTri);
int markPositionsToHost(pt_ctx* on);   // mark.tri from mark.dTri, for a mark whose records were made on the device

int buildScene(pt_ctx* c) {
    SceneBuffers* host = nullptr;
    if (const int rc = settledScene(c, &host)) return rc;
    const SceneBuffers& b = *host;
    SceneLayout L; std::string err;
    if (const int rc = layoutScene(b, c->opt, L, err)) return fail(rc, err);
    hipStream_t s = c->stream;
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(c->dNodes.upload(L.nodes.data(), L.nodes.size() * 16, s));
    HIP_TRY(c->dNodes80.upload(L.nodes80.data(), L.nodes80.size() * 4, s));
    HIP_TRY(c->dTris.upload(L.tris.data(), L.tris.size() * 16, s));
    HIP_TRY(c->dShade.upload(L.shade.data(), L.shade.size() * 16, s));
    HIP_TRY(c->dTriObj.upload(L.triObj.data(), L.triObj.size() * 4, s));
    HIP_TRY(c->dRoots.upload(L.roots.data(), L.roots.size() * sizeof(ObjRoot), s));
    HIP_TRY(c->dEllip.upload(L.ellip.data(), L.ellip.size() * sizeof(EllipRec), s));
    HIP_TRY(c->dMats.upload(L.mats.data(), L.mats.size() * sizeof(MatRec), s));
    HIP_TRY(c->dMatVD.upload(L.matVD.data(), L.matVD.size(), s));
    HIP_TRY(c->dSky.upload(b.sky.data(), (size_t)b.skyW * b.skyH * 4, s));
    HIP_TRY(c->dNiTable.upload(L.niDict.data(), L.niDict.size() * 4, s));
    // the texture table beyond the sky: ONE allocation and one asynchronous copy for all textures; the table gets its device pointers once dTexels exists
    HIP_TRY(c->dTexels.upload(L.texels.data(), L.texels.size(), s));
    std::vector<TexRec> table(L.texOff.size());
    for (size_t ti = 0; ti < table.size(); ti++) {
        const bool present = ti > 0 && !b.textures[ti].rgba.empty();
        table[ti].data = ti == 0 ? (const uchar4*)c->dSky : present ? c->dTexels + L.texOff[ti] : nullptr; table[ti].w = L.texW[ti]; table[ti].h = L.texH[ti];
    }
    HIP_TRY(c->dTexTable.upload(table.data(), table.size() * sizeof(TexRec), s));
    HIP_TRY(hipStreamSynchronize(s));
    DevScene& sc = c->sc;
    sc.nodes = c->dNodes; sc.nNodes = L.nInner; sc.tris = c->dTris; sc.nTriRecs = L.nTriRecs;
    sc.shade = c->dShade; sc.nTris = L.nTris; sc.triObj = c->dTriObj; sc.roots = c->dRoots; sc.numObj = L.numObj; sc.ellip = c->dEllip; sc.numEllip = L.numEllip;
    for (int k = 0; k < 8; k++) sc.ni8[k] = L.ni8[k];
    sc.niTable = c->dNiTable;
    sc.mats = c->dMats; sc.numMat = L.numMat; sc.sky = c->dSky; sc.skyW = b.skyW; sc.skyH = b.skyH; sc.tex = c->dTexTable; sc.numTex = (int)table.size();
    sc.ldsNodes = L.ldsNodes; sc.ldsTris = L.ldsTris;
    c->trans = L.trans; c->anySubsurface = L.anySubsurface; c->anyMaps = L.anyMaps; c->ambiguousTriObj = L.ambiguousTriObj;
    c->niBits = L.niBits; c->asmGroupShift = L.asmGroupShift; c->asmWhyNot = L.asmWhyNot;
    c->built = L.planScene();
    c->sceneDirty = false;
    return 0;
}

int ensurePool(pt_ctx* c, int capacity) {               // capacity >= poolActive: room for a pool that grows while a stream runs
    capacity = std::max(capacity, c->sched.poolActive);
    if (c->allocSlots >= capacity && c->allocNiBits == c->niBits && c->allocHX == c->built.ellipMaps) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->allocSlots = 0;                                            // until every allocation below has succeeded there is no pool
    float4** groups[] = {&c->st.G0, &c->st.G1, &c->st.G2, &c->st.G3, &c->st.G4, &c->st.H, &c->st.G5, &c->st.S0, &c->st.HX};
    for (int k = 0; k < 9; k++) { *groups[k] = nullptr; HIP_TRY(c->dPool[k].release()); }
    c->st.J = nullptr;
    HIP_TRY(c->dPoolJ.release());
    for (auto& q : c->dQueue) HIP_TRY(q.release());
    size_t n = (size_t)capacity;
    for (int k = 0; k < 9; k++) {
        if ((k == 6 && c->niBits == 0) || (k == 7 && c->niBits < 8) || (k == 8 && !c->built.ellipMaps)) continue;      // G5: transmissive scenes; S0: 8-bit index-stack codes, or three planes of floats; HX: mapped ellipsoids
        HIP_TRY(c->dPool[k].reset(n * 16 * ((k == 7 && c->niBits == 32) ? 3 : 1)));
        *groups[k] = c->dPool[k];
    }
    HIP_TRY(c->dPoolJ.reset(n * 8));
    c->st.J = c->dPoolJ;
    if (!c->dZero) {
        HIP_TRY(c->dZero.reset(64));
        HIP_TRY(hipMemsetAsync(c->dZero, 0, 64, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));                 // the shading launches run on other streams as well
    }
    c->st.Z = c->dZero;
    for (auto& q : c->dQueue) HIP_TRY(q.reset(n * 4));
    c->allocSlots = capacity; c->allocNiBits = c->niBits; c->allocHX = c->built.ellipMaps; c->st.s0Plane = (unsigned)capacity;
    return 0;
}

// the frame inputs current at the call; false while Parameters, ORIGIN or ROTATION are not set
bool currentInputs(const pt_ctx* c, FrameIn& fin) {
    if (c->buf.params.size() < 12 || c->buf.origin.size() < 3 || c->buf.rotation.size() < 3 || c->buf.mouse.size() < 3) return false;
    std::memcpy(fin.params, c->buf.params.data(), 48); std::memcpy(fin.origin, c->buf.origin.data(), 12); std::memcpy(fin.rotation, c->buf.rotation.data(), 12);
    std::memcpy(fin.mouse, c->buf.mouse.data(), 12);
    return true;
}
// pt_write_frame, pt_reproject_frame: the current image's camera is the inputs current at the call (include/pt_reproject.h)
void recordCamera(pt_ctx* c) {
    FrameIn cur;
    c->hist.written(currentInputs(c, cur) ? &cur : nullptr);
}

// A single context's accumulator slots (FRAME or T) to and from a whole image in host pixel order, on k->stream, synchronised.  A whole-image
// context's slot of a pixel is the pixel (nLocal = nSlotsImg = W*H); a shard's slots follow its pixel list, zero-padded to nSlotsImg as pt_reset_frame
// leaves them.
int shardToHost(pt_ctx* k, const float4* devSlots, float* img) {
    const bool whole = k->shardCount == 1;
    std::vector<float> tmp(whole ? 0 : (size_t)k->nLocal * 4);
    HIP_TRY(hipMemcpyAsync(whole ? img : tmp.data(), devSlots, (size_t)k->nLocal * 16, hipMemcpyDeviceToHost, k->stream));
    HIP_TRY(hipStreamSynchronize(k->stream));
    for (int i = 0; !whole && i < k->nLocal; i++) std::memcpy(img + 4 * (size_t)k->pixList[i], tmp.data() + 4 * (size_t)i, 16);
    return 0;
}
int hostToShard(pt_ctx* k, const float* img, float4* devSlots) {
    const bool whole = k->shardCount == 1;
    std::vector<float> tmp(whole ? 0 : (size_t)k->nSlotsImg * 4, 0.0f);
    for (int i = 0; !whole && i < k->nLocal; i++) std::memcpy(tmp.data() + 4 * (size_t)i, img + 4 * (size_t)k->pixList[i], 16);
    HIP_TRY(hipMemcpyAsync(devSlots, whole ? img : tmp.data(), (size_t)k->nSlotsImg * 16, hipMemcpyHostToDevice, k->stream));
    HIP_TRY(hipStreamSynchronize(k->stream));
    return 0;
}

// T (per accumulator slot), allocated when a call first needs it: zeroed on the context's stream, or left for the caller to fill
int ensureStats(pt_ctx* c, bool zeroed) {
    if (c->dStats) return 0;
    HIP_TRY(c->dStats.ensure((size_t)c->nSlotsImg * 16));
    if (zeroed) HIP_TRY(hipMemsetAsync(c->dStats, 0, (size_t)c->nSlotsImg * 16, c->stream));
    return 0;
}

}  // namespace
