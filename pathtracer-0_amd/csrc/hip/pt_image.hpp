// pt_image.hpp — the host half of the image-space passes behind the C ABI (included by pt_hip.hip inside its extern "C" block, where pt_ctx and
// its helpers are in scope; not a translation unit).  T in pixel order, the feature and seen-through records, the a-trous and the variance-guided
// filter, the reprojection across camera moves (also through mirror and glass chains, and with bilinear taps) and moved geometry (also with bilinear taps), the history validation, steering and the prefill.  The kernels are pt_denoise.hip's, pt_guided.hip's
// and pt_reproject.hip's, behind pt_image_launch.hpp; the kernels of the records are pt_kernels.hpp's.

// ---- T in pixel order (include/pt_adaptive.h, include/pt_guided.h): a group's streams each hold the slots of their own shard, so T travels through the host
namespace {
// T of the whole image into host[W*H*4], pixel order: zeros where no stream holds T; *any = some stream does.  Work in flight is the caller's to complete.
int statsToHost(pt_ctx* c, float* host, bool* any) {
    std::fill(host, host + (size_t)c->W * c->H * 4, 0.0f);
    *any = false;
    const std::vector<pt_ctx*> kids = c->multi ? c->multi->kids : std::vector<pt_ctx*>{c};
    for (pt_ctx* k : kids) {
        if (!k->dStats) continue;
        *any = true;
        HIP_TRY(hipSetDevice(k->device));
        if (int rc = shardToHost(k, k->dStats, host)) return rc;
    }
    return 0;
}
// The whole image's T in pixel order on the device of `on` (firstStream(c)), or nullptr when no stream holds T: a single context's own T; a group's
// gathered through the host into on->dStatsWhole.  Work in flight is the caller's to complete.
int wholeStats(pt_ctx* c, pt_ctx* on, const float4** stats) {
    *stats = c->multi ? nullptr : c->dStats.p;
    if (!c->multi) return 0;
    const size_t n = (size_t)c->W * c->H;
    std::vector<float> host(n * 4);
    bool any = false;
    if (int rc = statsToHost(c, host.data(), &any)) return rc;
    if (!any) return 0;
    HIP_TRY(hipSetDevice(on->device));
    HIP_TRY(on->dStatsWhole.ensure(n * 16));
    HIP_TRY(hipMemcpyAsync(on->dStatsWhole, host.data(), n * 16, hipMemcpyHostToDevice, on->stream));
    HIP_TRY(hipStreamSynchronize(on->stream));
    *stats = on->dStatsWhole;
    return 0;
}
int writeMoments(pt_ctx* c, const float* in) {
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = flushStream(c)) return rc;
    if (int rc = ensureStats(c, false)) return rc;
    return hostToShard(c, in, c->dStats);
}
// every stream of the context synchronised: all submitted work has landed in FRAME and T
int syncAll(pt_ctx* c) {
    if (c->multi) return multiRun(*c->multi, [](pt_ctx* k) { return pt_synchronize(k); });
    return pt_synchronize(c);
}
// runs `call` with a count of its own and stores it, zero when the call fails before counting, into *out (may be NULL)
int counted(int64_t* out, const std::function<int(int64_t*)>& call) {
    int64_t n = 0;
    const int rc = call(&n);
    if (out) *out = n;
    return rc;
}
// ---- every entry point below asks its row of pt_image_args.hpp first: what it refuses in its arguments, in which order and in which words, is there
using ptp::ImageArgs;
using ptp::checkImageArgs;
const char* nameOf(ptp::ImageCall call) { return ptp::imageCallTable()[call].name; }
}  // namespace

int pt_record_moments(pt_ctx* c, int on) {
    if (int rc = fail(checkImageArgs(ptp::IC_RECORD_MOMENTS, ImageArgs::given(c)))) return rc;
    MULTI_ALL(c, pt_record_moments(k, on));
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = flushStream(c)) return rc;                       // batches in flight retire under the previous setting
    if (on) { if (int rc = ensureStats(c, true)) return rc; }
    c->recordMoments = on != 0;
    return PT_OK;
}

int pt_read_moments(pt_ctx* c, float* out) {
    int rc;
    if ((rc = fail(checkImageArgs(ptp::IC_READ_MOMENTS, ImageArgs::given(c, out))))) return rc;
    if ((rc = needWholeImage(c, PT_ERR_UNSUPPORTED, "pt_read_moments"))) return rc;
    if ((rc = pt_synchronize(c))) return rc;
    bool any = false;
    return statsToHost(c, out, &any);
}

int pt_write_moments(pt_ctx* c, const float* in) {
    if (int rc = fail(checkImageArgs(ptp::IC_WRITE_MOMENTS, ImageArgs::given(c, in)))) return rc;
    if (int rc = needWholeImage(c, PT_ERR_UNSUPPORTED, "pt_write_moments")) return rc;
    MULTI_ALL(c, writeMoments(k, in));                            // every stream takes the pixels of its own tile shard
    return writeMoments(c, in);
}

// ---- first-hit feature records and the denoised image (include/pt_denoise.h).  A group context works on its first stream's context: the scene is replicated.
namespace {
// The records of the frame inputs `fin` in the cache `which`: first-hit records (rule == nullptr), or the seen-through records under `rule` with their last
// segments.  Returns at once when it holds them; a failed fill leaves it invalid.  A probe pool takes the camera rays (k_feature_rays); then one
// intersect and k_feature_record, or max_depth + 1 rounds of (intersect, k_through_step) — a fixed count, nothing read back in between: a round
// whose lanes are all dead costs two launches that return at once
int ensureRecords(pt_ctx* c, ptp::RecordCache which, const FrameIn& fin, const pt_through_rule* rule, const char* who) {
    HIP_TRY(hipSetDevice(c->device));
    if (c->hist.cached(which, fin, rule)) return 0;
    c->hist.beginFill(which);
    pt_ctx::Records& R = c->rec[which];
    int rc;
    if ((rc = claimFrameConstants(c))) return rc;
    if (rule && (rule->flags & PT_THROUGH_KEY) && c->sc.numMat > 4096)
        return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": PT_THROUGH_KEY packs a material index into 12 bits; the scene has more than 4096 materials");
    const size_t n = (size_t)c->W * c->H, np = (n + BLOCK - 1) / BLOCK * BLOCK;
    HIP_TRY(R.recs.ensure(n * 64));
    if (rule) HIP_TRY(R.rays.ensure(n * 32));
    ProbePool pool;
    if ((rc = pool.alloc(np, c->sc.numEllip > 0))) return rc;      // HX: the uv an ellipsoid hit inherits (uvOfHit)
    const State& st = pool.st;
    Dev<float4> X;                                                // the chains' state between the rounds
    if (rule) HIP_TRY(X.ensure(np * 16 * (c->niBits == 32 ? 5 : (c->niBits == 8 ? 3 : 2))));
    if (st.HX) HIP_TRY(hipMemsetAsync(st.HX, 0, np * 16, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(c->dFrameIn, &fin, sizeof(fin), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_frame_setup, dim3(1), dim3(64), 0, c->stream, c->sc, c->dFrameIn, c->dFc, c->dEllip);      // auto-focus, camera and ellipsoid rotations
    hipLaunchKernelGGL(k_feature_rays, dim3((unsigned)(np / BLOCK)), dim3(BLOCK), 0, c->stream, (const FrameConst*)c->dFc, c->W, c->H, st, (int)np);
    if (!rule) {
        if ((rc = probeIntersect(c, st, np))) return rc;
        hipLaunchKernelGGL(k_feature_record, dim3((unsigned)(np / BLOCK)), dim3(BLOCK), 0, c->stream, c->sc, st, (int)n, R.recs.p);
    } else {
        // RAYTRACING == 0 (directDiffuse, frag.glsl:911-912) takes no step
        const int depth = (rule->lobes == 0 || fin.params[9] != 1.0f) ? 0 : rule->max_depth;
        const ThroughRule tr{depth, rule->min_weight, rule->lobes, rule->flags};
        for (int step = 0; step <= depth; step++) {
            if ((rc = probeIntersect(c, st, np))) return rc;
#define THROUGH_STEP(T) hipLaunchKernelGGL(k_through_step<T>, dim3((unsigned)(np / BLOCK)), dim3(BLOCK), 0, c->stream, c->sc, st, (int)n, tr, step, X.p, (unsigned)np, R.recs.p, R.rays.p)
            if (c->niBits == 3) THROUGH_STEP(3);
            else if (c->niBits == 8) THROUGH_STEP(8);
            else if (c->niBits == 32) THROUGH_STEP(32);
            else THROUGH_STEP(0);
#undef THROUGH_STEP
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->hist.filled(which, fin, rule);
    return 0;
}
// the records of the current frame inputs: RC_FEAT, or RC_THRU under `rule`
int currentRecords(pt_ctx* c, const pt_through_rule* rule, const char* who) {
    if (c->buf.params.size() < 12) return fail(PT_ERR_ARG, "Parameters (binding 4) not set");
    if (c->buf.origin.size() < 3 || c->buf.rotation.size() < 3) return fail(PT_ERR_ARG, "ORIGIN / ROTATION (bindings 0, 1) not set");
    FrameIn fin;
    currentInputs(c, fin);
    return ensureRecords(c, rule ? ptp::RC_THRU : ptp::RC_FEAT, fin, rule, who);
}

// the filters' scratch on the device of `on`: the colour ping-pong and the output (W*H float4 each), the packed guide (2*W*H float4)
int ensureFilterScratch(pt_ctx* on) {
    const size_t n = (size_t)on->W * on->H;
    for (Dev<float4>* p : {&on->dDnCol[0], &on->dDnCol[1], &on->dDnOut}) HIP_TRY(p->ensure(n * 16));
    HIP_TRY(on->dDnGuide.ensure(n * 32));
    return 0;
}
// an image a filter left on the device of `on` (W*H float4, written on on->stream) into rgba_out; with dCount, that count into *count
int imageToHost(pt_ctx* on, const float4* src, float* rgba_out, const unsigned* dCount = nullptr, int64_t* count = nullptr) {
    unsigned n = 0;
    HIP_TRY(hipMemcpyAsync(rgba_out, src, (size_t)on->W * on->H * 16, hipMemcpyDeviceToHost, on->stream));
    if (dCount) HIP_TRY(hipMemcpyAsync(&n, dCount, 4, hipMemcpyDeviceToHost, on->stream));
    HIP_TRY(hipStreamSynchronize(on->stream));
    if (count) *count = n;
    return PT_OK;
}
// on->dDnOut for the display.  A filtered image is a mean already: k_display's conversion with a frame count of 1 (x / 1.0f is exact)
int displayFiltered(pt_ctx* on, int java_bytes, uint8_t* rgb_out) {
    return displayInto(on, on->dDnOut, on->W, on->H, false, 1.0f, java_bytes, rgb_out);
}

// the denoised image of the context's current FRAME into on->dDnOut (W*H float4 on the device of *on), enqueued on on->stream
int denoiseImage(pt_ctx* c, int iterations, const float (&sigma)[4], pt_ctx** onOut) {
    pt_ctx* on = nullptr; const float4* frame = nullptr;
    int rc;
    if ((rc = wholeFrame(c, PT_ERR_UNSUPPORTED, "pt_denoise", &on, &frame))) return rc;
    if ((rc = currentRecords(on, nullptr, "pt_denoise"))) return rc;
    if ((rc = ensureFilterScratch(on))) return rc;
    on->filteredThere = false;
    HIP_TRY(denoiseLaunch(frame, on->rec[ptp::RC_FEAT].recs, c->W, c->H, iterations, sigma, on->dDnCol[0], on->dDnCol[1], on->dDnGuide, on->dDnOut, on->stream));
    on->filteredThere = true;
    *onOut = on;
    return 0;
}
}  // namespace

int pt_read_features(pt_ctx* c, float* out) {
    int rc;
    if ((rc = fail(checkImageArgs(ptp::IC_READ_FEATURES, ImageArgs::given(c, out))))) return rc;
    pt_ctx* on = firstStream(c);
    if ((rc = currentRecords(on, nullptr, "pt_read_features"))) return rc;
    HIP_TRY(hipMemcpy(out, on->rec[ptp::RC_FEAT].recs, (size_t)c->W * c->H * 64, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_denoise(pt_ctx* c, int iterations, float sigma_color, float sigma_normal, float sigma_depth, float sigma_albedo, float* rgba_out) {
    if (int rc = fail(checkImageArgs(ptp::IC_DENOISE, ImageArgs::given(c, rgba_out).filter(iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo, 0, 0.0f)))) return rc;
    pt_ctx* on = nullptr;
    if (int rc = denoiseImage(c, iterations, {sigma_color, sigma_normal, sigma_depth, sigma_albedo}, &on)) return rc;
    return imageToHost(on, on->dDnOut, rgba_out);
}

int pt_read_display_denoised(pt_ctx* c, int iterations, float sigma_color, float sigma_normal, float sigma_depth, float sigma_albedo, int java_bytes, uint8_t* rgb_out) {
    if (int rc = fail(checkImageArgs(ptp::IC_READ_DISPLAY_DENOISED, ImageArgs::given(c, rgb_out).filter(iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo, 0, 0.0f))))
        return rc;
    pt_ctx* on = nullptr;
    if (int rc = denoiseImage(c, iterations, {sigma_color, sigma_normal, sigma_depth, sigma_albedo}, &on)) return rc;
    return displayFiltered(on, java_bytes, rgb_out);
}

// ---- the variance-guided filter (include/pt_guided.h) and, in front of it, the prefill of the unrendered pixels (include/pt_fill.h): pt_denoise's
// plumbing and scratch, with T in pixel order beside FRAME, and FRAME' and the filled count beside them
namespace {
// Of the context's current image: when `fill`, FRAME' into on->dFill and the filled count into on->dFillCount; when `filter`, the guided filter over
// FRAME (or FRAME') into on->dDnOut.  All enqueued on on->stream.  sigma = (luminance, normal, depth, albedo); the luminance entry, iterations and
// minFrames count only when `filter`.  floorA == 0: the plain kernels; > 0: include/pt_demod.h's, with that albedo_floor.
// thru: null = the first-hit records; else include/pt_through.h's records under that rule in their place
int filteredImage(pt_ctx* c, bool fill, bool filter, int iterations, const float (&sigma)[4], int minFrames, float floorA, const char* who, pt_ctx** onOut,
                  const pt_through_rule* thru = nullptr) {
    const std::string w(who);
    pt_ctx* on = nullptr;
    GuidedJob j;
    int rc;
    if ((rc = wholeFrame(c, PT_ERR_UNSUPPORTED, who, &on, &j.frame))) return rc;
    if (filter) {
        if ((rc = wholeStats(c, on, &j.stats))) return rc;
        if (!j.stats) return fail(PT_ERR_ARG, w + ": the image has no luminance moments (T was never allocated): call pt_record_moments before rendering");
    }
    if ((rc = currentRecords(on, thru, who))) return rc;
    j.feat = thru ? on->rec[ptp::RC_THRU].recs : on->rec[ptp::RC_FEAT].recs;
    if ((rc = ensureFilterScratch(on))) return rc;
    if (fill) {
        HIP_TRY(on->dFill.ensure((size_t)c->W * c->H * 16));
        HIP_TRY(on->dFillCount.ensure(4));
        j.fill = on->dFill; j.fillCount = on->dFillCount;
    }
    j.W = c->W; j.H = c->H; j.iterations = iterations; j.minFrames = minFrames; j.floorA = floorA;
    std::copy(sigma, sigma + 4, j.sigma);
    j.col0 = on->dDnCol[0]; j.col1 = on->dDnCol[1]; j.guide = on->dDnGuide;
    if (filter) { j.out = on->dDnOut; on->filteredThere = false; }
    HIP_TRY(guidedLaunch(j, on->stream));
    if (filter) on->filteredThere = true;
    *onOut = on;
    return 0;
}
// pt_denoise_guided, its demodulated form (floorA > 0) and their display forms: the filtered image to the host (rgba_out) or to the display
// (rgb_out).  All four share the first one's message prefix past their own checks
int guidedTo(ptp::ImageCall call, pt_ctx* c, int iterations, const float (&sigma)[4], int minFrames, float floorA, float* rgba_out, int java_bytes, uint8_t* rgb_out) {
    if (int rc = fail(checkImageArgs(call, ImageArgs::given(c, rgba_out ? (const void*)rgba_out : rgb_out).filter(iterations, sigma[0], sigma[1], sigma[2], sigma[3], minFrames, floorA))))
        return rc;
    pt_ctx* on = nullptr;
    if (int rc = filteredImage(c, false, true, iterations, sigma, minFrames, floorA, "pt_denoise_guided", &on)) return rc;
    return rgba_out ? imageToHost(on, on->dDnOut, rgba_out) : displayFiltered(on, java_bytes, rgb_out);
}
}  // namespace

int pt_denoise_guided(pt_ctx* c, int iterations, float sigma_lum, float sigma_normal, float sigma_depth, float sigma_albedo, int min_frames, float* rgba_out) {
    return guidedTo(ptp::IC_DENOISE_GUIDED, c, iterations, {sigma_lum, sigma_normal, sigma_depth, sigma_albedo}, min_frames, 0.0f, rgba_out, 0, nullptr);
}

int pt_read_display_denoised_guided(pt_ctx* c, int iterations, float sigma_lum, float sigma_normal, float sigma_depth, float sigma_albedo, int min_frames,
                                    int java_bytes, uint8_t* rgb_out) {
    return guidedTo(ptp::IC_READ_DISPLAY_DENOISED_GUIDED, c, iterations, {sigma_lum, sigma_normal, sigma_depth, sigma_albedo}, min_frames, 0.0f, nullptr, java_bytes, rgb_out);
}

int pt_denoise_guided_demod(pt_ctx* c, int iterations, float sigma_lum, float sigma_normal, float sigma_depth, float sigma_albedo, int min_frames,
                            float albedo_floor, float* rgba_out) {
    return guidedTo(ptp::IC_DENOISE_GUIDED_DEMOD, c, iterations, {sigma_lum, sigma_normal, sigma_depth, sigma_albedo}, min_frames, albedo_floor, rgba_out, 0, nullptr);
}

int pt_read_display_denoised_guided_demod(pt_ctx* c, int iterations, float sigma_lum, float sigma_normal, float sigma_depth, float sigma_albedo,
                                          int min_frames, float albedo_floor, int java_bytes, uint8_t* rgb_out) {
    return guidedTo(ptp::IC_READ_DISPLAY_DENOISED_GUIDED_DEMOD, c, iterations, {sigma_lum, sigma_normal, sigma_depth, sigma_albedo}, min_frames, albedo_floor, nullptr,
                    java_bytes, rgb_out);
}

// ---- reprojection across a camera move (include/pt_reproject.h).  A group context reprojects its gathered image on its first stream's context and hands
// every stream its shard back through the host, as pt_write_frame distributes an image; T travels through the host both ways.
namespace {
// the current inputs of `on` into cur, refused unless they render surfaces at the image's size; toDo: what the caller wants surfaces for
int usableInputs(pt_ctx* on, const std::string& w, const char* toDo, FrameIn& cur) {
    return fail(on->hist.usableInputs(currentInputs(on, cur) ? &cur : nullptr, w, toDo));
}
// the reprojected image (on->dRpFrame, on->dRpStats when `stats`, on->dRpKept; enqueued on on->stream) into the current image of `c`, whose camera
// becomes the current inputs
int storeReprojected(pt_ctx* c, pt_ctx* on, bool stats, int64_t* nKept) {
    const size_t n = (size_t)c->W * c->H;
    int rc;
    unsigned kept = 0;
    HIP_TRY(hipMemcpyAsync(&kept, on->dRpKept, 4, hipMemcpyDeviceToHost, on->stream));
    if (!c->multi) {                                              // the result into the current image (a copy: pt_frame_device pointers stay valid)
        HIP_TRY(hipMemcpyAsync(c->dImage[c->hist.image()], on->dRpFrame, n * 16, hipMemcpyDeviceToDevice, c->stream));
        if (stats) HIP_TRY(hipMemcpyAsync(c->dStats, on->dRpStats, n * 16, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        recordCamera(c);
    } else {
        std::vector<float> hf(n * 4), hostStats(stats ? n * 4 : 0);
        HIP_TRY(hipMemcpyAsync(hf.data(), on->dRpFrame, n * 16, hipMemcpyDeviceToHost, on->stream));
        if (stats) HIP_TRY(hipMemcpyAsync(hostStats.data(), on->dRpStats, n * 16, hipMemcpyDeviceToHost, on->stream));
        HIP_TRY(hipStreamSynchronize(on->stream));
        const float* pf = hf.data(); const float* ps = stats ? hostStats.data() : nullptr;
        if ((rc = multiRun(*c->multi, [pf, ps](pt_ctx* k) { return writeFrame(k, pf, ps); }))) return rc;
    }
    *nKept = kept;
    return 0;
}
// ---- include/pt_motion.h: where the primitives are, for the mark and for the reprojection across moved geometry
// (pt_motion_pack.hpp turns the bound buffers and the mark's host copies into the records uploaded here)

// The image of `c` mapped to the current inputs, stored as its current image; *nKept = the pixels kept.  `moved`: include/pt_motion.h's call, with Rh
// and the primitives' old positions from the mark (which it spends); else include/pt_reproject.h's, Rh from the image's camera.
// floorA == 0: include/pt_reproject.h's step 7; > 0: include/pt_demod.h's, with that albedo_floor.
// chain (not moved, floorA 0): include/pt_reproject_through.h's call, Sn / Yn and Sh / Yh beside Rn and Rh
// taps (no chain): include/pt_reproject_bilinear.h's call, the four old pixels around the projected point; with `moved`, include/pt_motion_bilinear.h's
struct ChainCarry { const pt_through_rule* thru; float pointTol; int radius; int64_t* nKeptThrough; };
struct BilinearTaps { float snap; int64_t* nBlended; };
int reprojectImage(pt_ctx* c, const char* who, bool moved, float maxHistory, float depthTol, float normalTol, int flags, float floorA, int64_t* nKept,
                   const ChainCarry* chain = nullptr, const BilinearTaps* taps = nullptr) {
    const std::string w(who);
    pt_ctx* on = nullptr;
    ReprojectJob j;
    int rc;
    if ((rc = wholeFrame(c, PT_ERR_UNSUPPORTED, who, &on, &j.frame))) return rc;      // a group: gathered on on->stream
    if ((rc = syncAll(c))) return rc;                             // all submitted work lands in FRAME and T first
    FrameIn cur;
    if ((rc = usableInputs(on, w, "carry", cur))) return rc;
    const pt_ctx::Mark& m = on->mark;
    // include/pt_motion_bilinear.h leaves an image without a camera alone as the bilinear call does, when there is no mark either (planReproject has
    // no "nothing" among its moved outcomes: pt_reproject_frame_moved answers "no mark" there).  With a mark, its refusals are the moved call's
    if (moved && taps && !on->hist.camera().valid && !on->hist.markValid()) return PT_OK;
    const ptp::ReprojectPlan plan = on->hist.planReproject(cur, moved, w);
    if ((rc = fail(plan.refused))) return rc;
    if (plan.nothing) return PT_OK;                               // no camera: nothing to map from
    const FrameIn camIn = on->hist.camera().in;                   // the image's camera
    // Rn, in the scene as it is now (builds it when an upload is pending); Rh from the mark, or of the image's camera (the same records when it is unchanged)
    if ((rc = ensureRecords(on, ptp::RC_FEAT, cur, nullptr, who))) return rc;
    j.rn = on->rec[ptp::RC_FEAT].recs;
    if (chain) {                                                  // an unchanged camera uses one pair for both
        if ((rc = ensureRecords(on, ptp::RC_THRU, cur, chain->thru, who))) return rc;
        if (!plan.sameCam && (rc = ensureRecords(on, plan.sh, camIn, chain->thru, who))) return rc;
        j.sn = on->rec[ptp::RC_THRU].recs; j.yn = on->rec[ptp::RC_THRU].rays; j.sh = on->rec[plan.sh].recs; j.yh = on->rec[plan.sh].rays;
        j.pointTol = chain->pointTol; j.radius = chain->radius;
    }
    if (moved) {
        j.rh = on->mark.feat;
    } else {
        if (!plan.sameCam && (rc = ensureRecords(on, plan.rh, camIn, nullptr, who))) return rc;
        j.rh = on->rec[plan.rh].recs;
    }
    HIP_TRY(hipSetDevice(on->device));
    const size_t n = (size_t)c->W * c->H;
    HIP_TRY(on->dRpFrame.ensure(n * 16));
    HIP_TRY(on->dRpKept.ensure(8));
    if (chain) HIP_TRY(on->dRpPack.ensure(n * 32));
    j.pack = on->dRpPack;
    // the image's T in pixel order, when allocated (group: through the host)
    if ((rc = wholeStats(c, on, &j.stats))) return rc;
    if (j.stats) HIP_TRY(on->dRpStats.ensure(n * 16));
    // where the primitives are now, with the moved ones flagged
    std::vector<float> pt, pe;
    ReprojMotion g{};
    if (moved) {
        std::vector<float> tri, el; int nTri = 0, nEl = 0;
        if (on->behind) {
            // host copies behind a pose (include/pt_pose.h): the triangles' records are made where the posed binding 3 lies, against the mark's
            // device records; the ellipsoids stay on the host path
            if ((rc = poseMotionRecords(on, on->mark.dTri, m.nTri, on->dMoveTri, &nTri))) return rc;
            const std::vector<float> noTris; int zero = 0;
            ptp::motionPositions(noTris, on->buf.ellip, tri, &zero, el, &nEl);
            const ptp::MotionThen then{nullptr, 0, m.el.data(), m.nEl};
            ptp::motionPack(tri, 0, el, nEl, &then, pt, pe);
        } else {
            if (m.triOnDevice && (rc = markPositionsToHost(on))) return rc;      // a mark taken while they were behind
            SceneBuffers* host = nullptr;
            if ((rc = settledScene(on, &host))) return rc;        // (current: nothing is downloaded)
            ptp::motionPositions(host->tris, host->ellip, tri, &nTri, el, &nEl);
            const ptp::MotionThen then{m.tri.data(), m.nTri, m.el.data(), m.nEl};
            ptp::motionPack(tri, nTri, el, nEl, &then, pt, pe);
            HIP_TRY(on->dMoveTri.upload(pt.data(), pt.size() * 4, on->stream));
        }
        HIP_TRY(on->dMoveEl.upload(pe.data(), pe.size() * 4, on->stream));
        g = ReprojMotion{on->dMoveTri, m.dTri, nTri, m.nTri, on->dMoveEl, m.dEl, nEl, m.nEl};
        j.motion = &g;
    }
    // the image's camera as k_frame_setup builds it (of which only camRot, origin, screenSize, focalLength and screenHratio are read), in the frame
    // constants, which are no stream's afterwards
    *on->hFrameIn = camIn;
    HIP_TRY(hipMemcpyAsync(on->dFrameIn, on->hFrameIn, sizeof(FrameIn), hipMemcpyHostToDevice, on->stream));
    hipLaunchKernelGGL(k_frame_setup, dim3(1), dim3(64), 0, on->stream, on->sc, on->dFrameIn, on->dFc, on->dEllip);
    on->hist.frameConstantsTaken();
    j.hist = on->dFc; j.matVD = on->dMatVD; j.nMat = on->sc.numMat; j.W = c->W; j.H = c->H;
    j.cam = ReprojCam{{cur.origin[0], cur.origin[1], cur.origin[2]}, cur.mouse[0], cur.mouse[1], cur.params[2]};
    j.rule = ReprojRule{maxHistory, depthTol, normalTol, (flags & PT_REPROJECT_ALL_MATERIALS) ? 1 : 0};
    j.floorA = floorA;
    if (taps) { j.bilinear = true; j.snap = taps->snap; }
    j.outFrame = on->dRpFrame; j.outStats = j.stats ? on->dRpStats.p : nullptr; j.kept = on->dRpKept;
    HIP_TRY(reprojectLaunch(j, on->stream));
    if (moved) HIP_TRY(hipStreamSynchronize(on->stream));         // (pt / pe leave scope: their copies have landed)
    if (chain) {
        unsigned keptThrough = 0;
        HIP_TRY(hipMemcpyAsync(&keptThrough, on->dRpKept + 1, 4, hipMemcpyDeviceToHost, on->stream));
        HIP_TRY(hipStreamSynchronize(on->stream));
        *chain->nKeptThrough = keptThrough;
    }
    if (taps) {
        unsigned blended = 0;
        HIP_TRY(hipMemcpyAsync(&blended, on->dRpKept + 1, 4, hipMemcpyDeviceToHost, on->stream));
        HIP_TRY(hipStreamSynchronize(on->stream));
        *taps->nBlended = blended;
    }
    if ((rc = storeReprojected(c, on, j.stats != nullptr, nKept))) return rc;
    if (moved) on->hist.markSpent();
    return 0;
}
}  // namespace

int pt_reproject_frame(pt_ctx* c, float max_history, float depth_tol, float normal_tol, int flags, int64_t* n_kept) {
    return counted(n_kept, [&](int64_t* n) {
        if (int rc = fail(checkImageArgs(ptp::IC_REPROJECT_FRAME, ImageArgs::given(c).reproject(max_history, depth_tol, normal_tol, flags, 0.0f)))) return rc;
        return reprojectImage(c, "pt_reproject_frame", false, max_history, depth_tol, normal_tol, flags, 0.0f, n);
    });
}

int pt_reproject_frame_demod(pt_ctx* c, float max_history, float depth_tol, float normal_tol, int flags, float albedo_floor, int64_t* n_kept) {
    return counted(n_kept, [&](int64_t* n) {
        if (int rc = fail(checkImageArgs(ptp::IC_REPROJECT_FRAME_DEMOD, ImageArgs::given(c).reproject(max_history, depth_tol, normal_tol, flags, albedo_floor)))) return rc;
        return reprojectImage(c, "pt_reproject_frame", false, max_history, depth_tol, normal_tol, flags, albedo_floor, n);
    });
}

// ---- include/pt_reproject_through.h
int pt_reproject_frame_through(pt_ctx* c, const pt_through_rule* thru, const pt_reproject_through_rule* rule, int64_t* n_kept, int64_t* n_kept_through) {
    if (n_kept) *n_kept = 0;
    if (n_kept_through) *n_kept_through = 0;
    ImageArgs a = ImageArgs::given(c).has(ptp::AP_RULE, rule).has(thru);
    if (rule) { a.reproject(rule->max_history, rule->depth_tol, rule->normal_tol, rule->flags, 0.0f); a.radius = rule->radius; a.point_tol = rule->point_tol; }
    if (int rc = fail(checkImageArgs(ptp::IC_REPROJECT_FRAME_THROUGH, a))) return rc;
    int64_t n = 0, nt = 0;
    const ChainCarry chain{thru, rule->point_tol, rule->radius, &nt};
    const int rc = reprojectImage(c, "pt_reproject_frame_through", false, rule->max_history, rule->depth_tol, rule->normal_tol, rule->flags, 0.0f, &n, &chain);
    if (n_kept) *n_kept = n;
    if (n_kept_through) *n_kept_through = rc ? 0 : nt;
    return rc;
}

// ---- include/pt_reproject_bilinear.h
int pt_reproject_frame_bilinear(pt_ctx* c, const pt_reproject_bilinear_rule* rule, int64_t* n_kept, int64_t* n_blended) {
    if (n_kept) *n_kept = 0;
    if (n_blended) *n_blended = 0;
    ImageArgs a = ImageArgs::given(c).has(ptp::AP_RULE, rule);
    if (rule) { a.reproject(rule->max_history, rule->depth_tol, rule->normal_tol, rule->flags, rule->albedo_floor); a.snap = rule->snap; }
    if (int rc = fail(checkImageArgs(ptp::IC_REPROJECT_FRAME_BILINEAR, a))) return rc;
    int64_t n = 0, nb = 0;
    const BilinearTaps taps{rule->snap, &nb};
    const int rc = reprojectImage(c, "pt_reproject_frame_bilinear", false, rule->max_history, rule->depth_tol, rule->normal_tol, rule->flags,
                                  rule->albedo_floor, &n, nullptr, &taps);
    if (n_kept) *n_kept = n;
    if (n_blended) *n_blended = rc ? 0 : nb;
    return rc;
}

// ---- include/pt_motion.h: the mark
namespace {
int motionMark(pt_ctx* c) {
    int rc;
    if ((rc = needWholeImage(c, PT_ERR_UNSUPPORTED, "pt_motion_mark"))) return rc;
    if ((rc = syncAll(c))) return rc;                             // all submitted work lands first
    pt_ctx* on = firstStream(c);
    if ((rc = fail(on->hist.takeMark()))) return rc;              // (the old mark is gone from here)
    // (a) Rh, through the cache pt_reproject_frame keeps, into a buffer that later uploads leave alone
    if ((rc = ensureRecords(on, ptp::RC_FEAT_H, FrameIn(on->hist.camera().in), nullptr, "pt_motion_mark"))) return rc;
    const size_t n = (size_t)c->W * c->H;
    pt_ctx::Mark& m = on->mark;
    HIP_TRY(m.feat.ensure(n * 64));
    HIP_TRY(hipMemcpyAsync(m.feat, on->rec[ptp::RC_FEAT_H].recs, n * 64, hipMemcpyDeviceToDevice, on->stream));
    // (b), (c) where the primitives are
    std::vector<float> pt, pe;
    if (on->behind) {
        // host copies behind a pose (include/pt_pose.h): motionPack's triangle records are made on the device from the posed binding 3; the host
        // positions are fetched from them if a later reprojection finds the host copies current again
        if ((rc = poseMotionRecords(on, nullptr, 0, m.dTri, &m.nTri))) return rc;
        m.tri.clear(); m.triOnDevice = true;
        const std::vector<float> noTris; std::vector<float> noPos; int zero = 0;
        ptp::motionPositions(noTris, on->buf.ellip, noPos, &zero, m.el, &m.nEl);
        ptp::motionPack(noPos, 0, m.el, m.nEl, nullptr, pt, pe);
    } else {
        SceneBuffers* host = nullptr;
        if ((rc = settledScene(on, &host))) return rc;            // (current: nothing is downloaded)
        ptp::motionPositions(host->tris, host->ellip, m.tri, &m.nTri, m.el, &m.nEl);
        ptp::motionPack(m.tri, m.nTri, m.el, m.nEl, nullptr, pt, pe);
        HIP_TRY(m.dTri.upload(pt.data(), pt.size() * 4, on->stream));
        m.triOnDevice = false;
    }
    HIP_TRY(m.dEl.upload(pe.data(), pe.size() * 4, on->stream));
    HIP_TRY(hipStreamSynchronize(on->stream));
    on->hist.markTaken();                                         // (d)
    return PT_OK;
}

}  // namespace

int pt_motion_mark(pt_ctx* c) {
    if (int rc = fail(checkImageArgs(ptp::IC_MOTION_MARK, ImageArgs::given(c)))) return rc;
    return motionMark(c);
}

int pt_reproject_frame_moved(pt_ctx* c, float max_history, float depth_tol, float normal_tol, int flags, float albedo_floor, int64_t* n_kept) {
    return counted(n_kept, [&](int64_t* n) {
        if (int rc = fail(checkImageArgs(ptp::IC_REPROJECT_FRAME_MOVED, ImageArgs::given(c).reproject(max_history, depth_tol, normal_tol, flags, albedo_floor)))) return rc;
        return reprojectImage(c, "pt_reproject_frame_moved", true, max_history, depth_tol, normal_tol, flags, albedo_floor, n);
    });
}

// ---- include/pt_motion_bilinear.h: the bilinear call's argument checks under this call's name, the moved call's path with the taps
int pt_reproject_frame_moved_bilinear(pt_ctx* c, const pt_reproject_bilinear_rule* rule, int64_t* n_kept, int64_t* n_blended) {
    if (n_kept) *n_kept = 0;
    if (n_blended) *n_blended = 0;
    ImageArgs a = ImageArgs::given(c).has(ptp::AP_RULE, rule);
    if (rule) { a.reproject(rule->max_history, rule->depth_tol, rule->normal_tol, rule->flags, rule->albedo_floor); a.snap = rule->snap; }
    if (int rc = fail(checkImageArgs(ptp::IC_REPROJECT_FRAME_BILINEAR, a, "pt_reproject_frame_moved_bilinear"))) return rc;
    int64_t n = 0, nb = 0;
    const BilinearTaps taps{rule->snap, &nb};
    const int rc = reprojectImage(c, "pt_reproject_frame_moved_bilinear", true, rule->max_history, rule->depth_tol, rule->normal_tol, rule->flags,
                                  rule->albedo_floor, &n, nullptr, &taps);
    if (n_kept) *n_kept = rc ? 0 : n;
    if (n_blended) *n_blended = rc ? 0 : nb;
    return rc;
}

// ---- history validation (include/pt_validate.h): the hold lives on the first stream's context, where the merge runs; a group's image and T travel
// as they do for the reprojection
namespace {
int historyHold(pt_ctx* c) {
    int rc;
    if ((rc = needWholeImage(c, PT_ERR_UNSUPPORTED, "pt_history_hold"))) return rc;
    if ((rc = syncAll(c))) return rc;                             // all submitted work lands in FRAME and T first
    pt_ctx* on = nullptr;
    const float4* frame = nullptr; const float4* stats = nullptr;
    if ((rc = wholeFrame(c, PT_ERR_UNSUPPORTED, "pt_history_hold", &on, &frame))) return rc;
    if ((rc = wholeStats(c, on, &stats))) return rc;
    if (!stats) return fail(PT_ERR_ARG, "pt_history_hold: the image has no luminance moments (T was never allocated): call pt_record_moments before rendering");
    if ((rc = fail(on->hist.takeHold()))) return rc;
    HIP_TRY(hipSetDevice(on->device));
    const size_t n = (size_t)c->W * c->H;
    HIP_TRY(on->hold.frame.ensure(n * 16));
    HIP_TRY(on->hold.stats.ensure(n * 16));
    on->hist.holdBegins();
    HIP_TRY(hipMemcpyAsync(on->hold.frame, frame, n * 16, hipMemcpyDeviceToDevice, on->stream));
    HIP_TRY(hipMemcpyAsync(on->hold.stats, stats, n * 16, hipMemcpyDeviceToDevice, on->stream));
    HIP_TRY(hipStreamSynchronize(on->stream));
    auto zero = [](pt_ctx* k) {                                   // the image and T alone: the camera records, camWrites and a mark stay
        HIP_TRY(hipSetDevice(k->device));
        HIP_TRY(hipMemsetAsync(k->dImage[k->hist.image()], 0, (size_t)k->nSlotsImg * 16, k->stream));
        if (k->dStats) HIP_TRY(hipMemsetAsync(k->dStats, 0, (size_t)k->nSlotsImg * 16, k->stream));
        HIP_TRY(hipStreamSynchronize(k->stream));
        return 0;
    };
    if (c->multi) { if ((rc = multiRun(*c->multi, zero))) return rc; }
    else if ((rc = zero(c))) return rc;
    on->hist.holdTaken();
    return PT_OK;
}

int historyMerge(pt_ctx* c, const pt_validate_rule& r, float* kappaOut, int64_t* nReduced) {
    int rc;
    if ((rc = syncAll(c))) return rc;                             // work in flight lands in FRAME and T first
    pt_ctx* on = firstStream(c);
    if ((rc = fail(on->hist.mergeHold()))) return rc;
    FrameIn cur;
    if ((rc = usableInputs(on, "pt_history_merge", "compare on", cur))) return rc;
    ValidateJob j;
    if ((rc = wholeFrame(c, PT_ERR_UNSUPPORTED, "pt_history_merge", &on, &j.frame))) return rc;      // a group: gathered on on->stream
    if ((rc = wholeStats(c, on, &j.stats))) return rc;
    if (!j.stats) return fail(PT_ERR_ARG, "pt_history_merge: the image has no luminance moments");
    if ((rc = currentRecords(on, nullptr, "pt_history_merge"))) return rc;
    HIP_TRY(hipSetDevice(on->device));
    const size_t n = (size_t)c->W * c->H;
    HIP_TRY(on->dRpFrame.ensure(n * 16));
    HIP_TRY(on->dRpStats.ensure(n * 16));
    HIP_TRY(on->dRpKept.ensure(8));
    if (kappaOut) HIP_TRY(on->dKappa.ensure(n * 4));
    j.feat = on->rec[ptp::RC_FEAT].recs; j.heldFrame = on->hold.frame; j.heldStats = on->hold.stats;
    j.W = c->W; j.H = c->H; j.radius = r.radius; j.zLo = r.z_lo; j.zHi = r.z_hi; j.normalTol = r.normal_tol;
    j.overlay[0] = cur.mouse[0]; j.overlay[1] = cur.mouse[1]; j.overlay[2] = cur.params[2];
    j.outFrame = on->dRpFrame; j.outStats = on->dRpStats; j.kappa = kappaOut ? on->dKappa.p : nullptr; j.reduced = on->dRpKept;
    HIP_TRY(validateLaunch(j, on->stream));
    if (kappaOut) HIP_TRY(hipMemcpyAsync(kappaOut, on->dKappa, n * 4, hipMemcpyDeviceToHost, on->stream));
    if ((rc = storeReprojected(c, on, true, nReduced))) return rc;      // (records the same camera again)
    HIP_TRY(hipStreamSynchronize(on->stream));
    on->hist.holdSpent();
    return 0;
}
}  // namespace

int pt_history_hold(pt_ctx* c) {
    if (int rc = fail(checkImageArgs(ptp::IC_HISTORY_HOLD, ImageArgs::given(c)))) return rc;
    return historyHold(c);
}

int pt_history_merge(pt_ctx* c, const pt_validate_rule* rule, float* kappa_out, int64_t* n_reduced) {
    return counted(n_reduced, [&](int64_t* n) {
        if (int rc = fail(checkImageArgs(ptp::IC_HISTORY_MERGE, ImageArgs::given(c).has(rule)))) return rc;
        return historyMerge(c, *rule, kappa_out, n);
    });
}


// ---- adaptive sampling steered by the guided filter (include/pt_steer.h).  The selection needs the whole image (the filter's plumbing: wholeFrame,
// wholeStats, currentRecords on the first stream's context); the render takes each stream's own pixels from the W*H-byte mask.
namespace {
size_t maskBytes(const pt_ctx* c) { return ((size_t)c->W * c->H + 3) & ~(size_t)3; }      // the active count follows, 4-byte aligned

// The rule over the context's current image into (*onOut)->dSelMask (W*H bytes, pixel order, on the device of firstStream(c)); *nActive = its count.
// FRAME and T are not modified; T never allocated reads as zeros (the filter's scratch output, zeroed).
// floorA == 0: include/pt_steer.h's rule; > 0: include/pt_demod.h's step 5, with that albedo_floor.
int selectGuided(pt_ctx* c, const pt_guided_rule& r, float floorA, const char* who, pt_ctx** onOut, int64_t* nActive) {
    pt_ctx* on = nullptr;
    GuidedJob j;
    int rc;
    if ((rc = wholeFrame(c, PT_ERR_UNSUPPORTED, who, &on, &j.frame))) return rc;
    if ((rc = wholeStats(c, on, &j.stats))) return rc;
    if ((rc = currentRecords(on, nullptr, who))) return rc;       // (Parameters, ORIGIN and ROTATION are set from here on)
    HIP_TRY(hipSetDevice(on->device));
    if ((rc = ensureFilterScratch(on))) return rc;
    HIP_TRY(on->dSelMask.ensure(maskBytes(on) + 4));
    if (!j.stats) {
        on->filteredThere = false;
        HIP_TRY(hipMemsetAsync(on->dDnOut, 0, (size_t)c->W * c->H * 16, on->stream));
        j.stats = on->dDnOut;
    }
    unsigned* count = reinterpret_cast<unsigned*>(on->dSelMask + maskBytes(on));
    const AdaptRule ovr = withOverlay(on, AdaptRule{});
    j.feat = on->rec[ptp::RC_FEAT].recs; j.W = c->W; j.H = c->H; j.iterations = r.iterations; j.minFrames = r.min_frames; j.floorA = floorA;
    j.sigma[0] = r.sigma_lum; j.sigma[1] = r.sigma_normal; j.sigma[2] = r.sigma_depth; j.sigma[3] = r.sigma_albedo;
    j.col0 = on->dDnCol[0]; j.col1 = on->dDnCol[1]; j.guide = on->dDnGuide;
    j.mask = on->dSelMask; j.count = count; j.maxFrames = r.max_frames; j.relErr = r.rel_err; j.absErr = r.abs_err;
    j.overlay[0] = ovr.mouseX; j.overlay[1] = ovr.mouseY; j.overlay[2] = ovr.resolution;
    HIP_TRY(guidedLaunch(j, on->stream));
    unsigned hc = 0;
    HIP_TRY(hipMemcpyAsync(&hc, count, 4, hipMemcpyDeviceToHost, on->stream));
    HIP_TRY(hipStreamSynchronize(on->stream));
    *nActive = hc;
    *onOut = on;
    return 0;
}

// pt_render_mask on one stream: hostMask (W*H bytes) into c->dSelMask, or, when hostMask is null, the mask already there (pt_render_adaptive_guided
// on a one-stream context); then the frame stream over the list entries it selects
int renderMask(pt_ctx* c, int firstFrame, int nFrames, const int32_t* seeds, const uint8_t* hostMask, const char* who, int64_t* nActive) {
    return renderSelected(c, firstFrame, nFrames, seeds, who, [c, hostMask](hipStream_t s, int nb) {
        if (hostMask) {
            HIP_TRY(c->dSelMask.ensure(maskBytes(c) + 4));
            HIP_TRY(hipMemcpyAsync(c->dSelMask, hostMask, (size_t)c->W * c->H, hipMemcpyHostToDevice, s));
        }
        hipLaunchKernelGGL(k_adaptive_select_mask, dim3(nb), dim3(BLOCK), 0, s, (const unsigned*)c->dPixXY, c->nLocal, c->W, (const unsigned char*)c->dSelMask,
                           withOverlay(c, AdaptRule{}), c->dAdaptFlag, c->dAdaptBlk);
        return 0;
    }, nActive);
}
}  // namespace

int pt_render_mask(pt_ctx* c, int first_frame, int n_frames, const int32_t* seeds, const uint8_t* mask, int64_t* n_active) {
    if (n_active) *n_active = 0;
    if (int rc = fail(checkImageArgs(ptp::IC_RENDER_MASK, ImageArgs::given(c).has(ptp::AP_MASK, mask).seeded(seeds, n_frames)))) return rc;
    return onEveryStream(c, [=](pt_ctx* k, int64_t* n) { return renderMask(k, first_frame, n_frames, seeds, mask, "pt_render_mask", n); }, n_active);
}

namespace {
// pt_select_guided (floorA == 0) and pt_select_guided_demod
int selectInto(ptp::ImageCall call, pt_ctx* c, const pt_guided_rule* rule, float floorA, uint8_t* mask_out, int64_t* n_active) {
    if (n_active) *n_active = 0;
    int rc;
    if ((rc = fail(checkImageArgs(call, ImageArgs::given(c, mask_out).has(rule).floor(floorA))))) return rc;
    pt_ctx* on = nullptr; int64_t n = 0;
    if ((rc = selectGuided(c, *rule, floorA, nameOf(call), &on, &n))) return rc;
    HIP_TRY(hipMemcpyAsync(mask_out, on->dSelMask, (size_t)c->W * c->H, hipMemcpyDeviceToHost, on->stream));
    HIP_TRY(hipStreamSynchronize(on->stream));
    if (n_active) *n_active = n;
    return PT_OK;
}

// pt_render_adaptive_guided (floorA == 0) and pt_render_adaptive_guided_demod
int renderAdaptiveGuided(ptp::ImageCall call, pt_ctx* c, int first_frame, int n_frames, const int32_t* seeds, const pt_guided_rule* rule, float floorA,
                         int64_t* n_active) {
    if (n_active) *n_active = 0;
    int rc;
    if ((rc = fail(checkImageArgs(call, ImageArgs::given(c).has(rule).seeded(seeds, n_frames).floor(floorA))))) return rc;
    const char* who = nameOf(call);
    const pt_ctx* f = firstStream(c);
    if (f->buf.params.size() >= 12 && f->buf.params[10] != 0.0f)          // before the selection, as renderSelected would after it
        return fail(PT_ERR_UNSUPPORTED, std::string(who) + ": DEBUG != 0 renders the traversal heat map, which has no noise to adapt to");
    pt_ctx* on = nullptr; int64_t n = 0;
    if ((rc = selectGuided(c, *rule, floorA, who, &on, &n))) return rc;
    if (!c->multi)                                                // one stream (holds the whole image): on == c, the mask stays in c->dSelMask
        return onEveryStream(c, [=](pt_ctx* k, int64_t* cnt) { return renderMask(k, first_frame, n_frames, seeds, nullptr, who, cnt); }, n_active);
    std::vector<uint8_t> host((size_t)c->W * c->H);               // a group: every stream selects from its own copy
    HIP_TRY(hipMemcpyAsync(host.data(), on->dSelMask, host.size(), hipMemcpyDeviceToHost, on->stream));
    HIP_TRY(hipStreamSynchronize(on->stream));
    const uint8_t* hm = host.data();
    return onEveryStream(c, [=](pt_ctx* k, int64_t* cnt) { return renderMask(k, first_frame, n_frames, seeds, hm, who, cnt); }, n_active);
}
}  // namespace

int pt_select_guided(pt_ctx* c, const pt_guided_rule* rule, uint8_t* mask_out, int64_t* n_active) {
    return selectInto(ptp::IC_SELECT_GUIDED, c, rule, 0.0f, mask_out, n_active);
}

int pt_render_adaptive_guided(pt_ctx* c, int first_frame, int n_frames, const int32_t* seeds, const pt_guided_rule* rule, int64_t* n_active) {
    return renderAdaptiveGuided(ptp::IC_RENDER_ADAPTIVE_GUIDED, c, first_frame, n_frames, seeds, rule, 0.0f, n_active);
}

int pt_select_guided_demod(pt_ctx* c, const pt_guided_rule* rule, float albedo_floor, uint8_t* mask_out, int64_t* n_active) {
    return selectInto(ptp::IC_SELECT_GUIDED_DEMOD, c, rule, albedo_floor, mask_out, n_active);
}

int pt_render_adaptive_guided_demod(pt_ctx* c, int first_frame, int n_frames, const int32_t* seeds, const pt_guided_rule* rule, float albedo_floor,
                                    int64_t* n_active) {
    return renderAdaptiveGuided(ptp::IC_RENDER_ADAPTIVE_GUIDED_DEMOD, c, first_frame, n_frames, seeds, rule, albedo_floor, n_active);
}

// ---- interleaved rendering (include/pt_fill.h): pt_render_mask over a lattice mask that every stream builds on its own device, and the prefill of
// the unrendered pixels in front of the guided filter (its plumbing and scratch, with FRAME' and the filled count beside them)
namespace {
int renderLattice(pt_ctx* c, int firstFrame, int nFrames, const int32_t* seeds, int stride, int phaseX, int phaseY, int64_t* nActive) {
    return renderSelected(c, firstFrame, nFrames, seeds, "pt_render_interleaved", [=](hipStream_t s, int nb) {
        HIP_TRY(c->dSelMask.ensure(maskBytes(c) + 4));
        const int n = c->W * c->H;
        hipLaunchKernelGGL(k_lattice_mask, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, c->dSelMask, c->W, n, stride, phaseX, phaseY);
        hipLaunchKernelGGL(k_adaptive_select_mask, dim3(nb), dim3(BLOCK), 0, s, (const unsigned*)c->dPixXY, c->nLocal, c->W, (const unsigned char*)c->dSelMask,
                           withOverlay(c, AdaptRule{}), c->dAdaptFlag, c->dAdaptBlk);
        return 0;
    }, nActive);
}

// pt_fill_frame and pt_fill_frame_through: FRAME' and the count of the holes filled, to the host
int fillTo(ptp::ImageCall call, pt_ctx* c, const pt_through_rule* thru, float sigmaNormal, float sigmaDepth, float sigmaAlbedo, float floorA, float* rgba_out,
           int64_t* n_filled) {
    if (n_filled) *n_filled = 0;
    if (int rc = fail(checkImageArgs(call, ImageArgs::given(c, rgba_out).has(thru).filter(0, 1.0f, sigmaNormal, sigmaDepth, sigmaAlbedo, 2, floorA)))) return rc;
    pt_ctx* on = nullptr;
    if (int rc = filteredImage(c, true, false, 0, {1.0f, sigmaNormal, sigmaDepth, sigmaAlbedo}, 2, floorA, nameOf(call), &on, thru)) return rc;
    return imageToHost(on, on->dFill, rgba_out, on->dFillCount, n_filled);
}
// pt_denoise_guided_filled, pt_denoise_guided_through and their display forms: the filter over FRAME', to the host (rgba_out) or to the display (rgb_out)
int filledTo(ptp::ImageCall call, pt_ctx* c, const pt_through_rule* thru, int iterations, const float (&sigma)[4], int minFrames, float floorA, float* rgba_out,
             int java_bytes, uint8_t* rgb_out) {
    const void* out = rgba_out ? (const void*)rgba_out : rgb_out;
    if (int rc = fail(checkImageArgs(call, ImageArgs::given(c, out).has(thru).filter(iterations, sigma[0], sigma[1], sigma[2], sigma[3], minFrames, floorA)))) return rc;
    pt_ctx* on = nullptr;
    if (int rc = filteredImage(c, true, true, iterations, sigma, minFrames, floorA, nameOf(call), &on, thru)) return rc;
    return rgba_out ? imageToHost(on, on->dDnOut, rgba_out) : displayFiltered(on, java_bytes, rgb_out);
}
// pt_read_features_through (the records) and pt_read_through_rays (their last segments, `rays`), to the host
int throughToHost(ptp::ImageCall call, pt_ctx* c, const pt_through_rule* rule, bool rays, float* out) {
    int rc;
    if ((rc = fail(checkImageArgs(call, ImageArgs::given(c, out).has(rule))))) return rc;
    pt_ctx* on = firstStream(c);
    if ((rc = currentRecords(on, rule, nameOf(call)))) return rc;
    const pt_ctx::Records& R = on->rec[ptp::RC_THRU];
    HIP_TRY(hipMemcpy(out, rays ? (const void*)R.rays.p : (const void*)R.recs.p, (size_t)c->W * c->H * (rays ? 32 : 64), hipMemcpyDeviceToHost));
    return PT_OK;
}
}  // namespace

int pt_render_interleaved(pt_ctx* c, int first_frame, int n_frames, const int32_t* seeds, int stride, int phase_x, int phase_y, int64_t* n_active) {
    if (n_active) *n_active = 0;
    if (int rc = fail(checkImageArgs(ptp::IC_RENDER_INTERLEAVED, ImageArgs::given(c).seeded(seeds, n_frames).lattice(stride, phase_x, phase_y)))) return rc;
    return onEveryStream(c, [=](pt_ctx* k, int64_t* n) { return renderLattice(k, first_frame, n_frames, seeds, stride, phase_x, phase_y, n); }, n_active);
}

int pt_fill_frame(pt_ctx* c, float sigma_normal, float sigma_depth, float sigma_albedo, float albedo_floor, float* rgba_out, int64_t* n_filled) {
    return fillTo(ptp::IC_FILL_FRAME, c, nullptr, sigma_normal, sigma_depth, sigma_albedo, albedo_floor, rgba_out, n_filled);
}

int pt_denoise_guided_filled(pt_ctx* c, int iterations, float sigma_lum, float sigma_normal, float sigma_depth, float sigma_albedo, int min_frames,
                             float albedo_floor, float* rgba_out) {
    return filledTo(ptp::IC_DENOISE_GUIDED_FILLED, c, nullptr, iterations, {sigma_lum, sigma_normal, sigma_depth, sigma_albedo}, min_frames, albedo_floor, rgba_out, 0,
                    nullptr);
}

int pt_read_display_denoised_guided_filled(pt_ctx* c, int iterations, float sigma_lum, float sigma_normal, float sigma_depth, float sigma_albedo,
                                           int min_frames, float albedo_floor, int java_bytes, uint8_t* rgb_out) {
    return filledTo(ptp::IC_READ_DISPLAY_DENOISED_GUIDED_FILLED, c, nullptr, iterations, {sigma_lum, sigma_normal, sigma_depth, sigma_albedo}, min_frames, albedo_floor,
                    nullptr, java_bytes, rgb_out);
}

// ---- seen-through feature records (include/pt_through.h): the records beside the first-hit ones, and include/pt_fill.h's calls on them
int pt_read_features_through(pt_ctx* c, const pt_through_rule* rule, float* out) {
    return throughToHost(ptp::IC_READ_FEATURES_THROUGH, c, rule, false, out);
}

int pt_read_through_rays(pt_ctx* c, const pt_through_rule* rule, float* out) {
    return throughToHost(ptp::IC_READ_THROUGH_RAYS, c, rule, true, out);
}

int pt_fill_frame_through(pt_ctx* c, const pt_through_rule* rule, float sigma_normal, float sigma_depth, float sigma_albedo, float albedo_floor,
                          float* rgba_out, int64_t* n_filled) {
    return fillTo(ptp::IC_FILL_FRAME_THROUGH, c, rule, sigma_normal, sigma_depth, sigma_albedo, albedo_floor, rgba_out, n_filled);
}

int pt_denoise_guided_through(pt_ctx* c, const pt_through_rule* rule, int iterations, float sigma_lum, float sigma_normal, float sigma_depth,
                              float sigma_albedo, int min_frames, float albedo_floor, float* rgba_out) {
    return filledTo(ptp::IC_DENOISE_GUIDED_THROUGH, c, rule, iterations, {sigma_lum, sigma_normal, sigma_depth, sigma_albedo}, min_frames, albedo_floor, rgba_out, 0,
                    nullptr);
}

int pt_read_display_denoised_guided_through(pt_ctx* c, const pt_through_rule* rule, int iterations, float sigma_lum, float sigma_normal,
                                            float sigma_depth, float sigma_albedo, int min_frames, float albedo_floor, int java_bytes, uint8_t* rgb_out) {
    return filledTo(ptp::IC_READ_DISPLAY_DENOISED_GUIDED_THROUGH, c, rule, iterations, {sigma_lum, sigma_normal, sigma_depth, sigma_albedo}, min_frames, albedo_floor,
                    nullptr, java_bytes, rgb_out);
}

// the in-place move of a scene's triangles (include/pt_move.h) and the read-back of the scene's record arrays
#include "pt_move_host.hpp"

// triangles animated by per-part matrices on the device (include/pt_pose.h), on the in-place move's path
#include "pt_pose_host.hpp"

// a joint hierarchy, keyed clips and their layered mix making a pose's records on the device (include/pt_rig.h, include/pt_rig_mix.h)
#include "pt_rig_host.hpp"

// the pose family's timers and readers of include/pt_debug.h
#include "pt_geom_debug_host.hpp"

// the outlier rejection (include/pt_despeckle.h): both calls on historyMerge's path
#include "pt_despeckle_host.hpp"

// the display image (include/pt_tonemap.h): metered exposure, tone curve and sRGB transfer on pt_read_display_mean's path
#include "pt_tonemap_host.hpp"

// ---- the glare and the display image of a device-resident image (include/pt_bloom.h)
#include "pt_bloom_host.hpp"
