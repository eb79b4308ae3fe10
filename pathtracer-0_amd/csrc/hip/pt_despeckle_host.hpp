// pt_despeckle_host.hpp — the host half of pt_despeckle and pt_despeckle_frame (include/pt_despeckle.h), behind the C ABI (included at the end of
// pt_image.hpp, inside pt_hip.hip's extern "C" block, where pt_ctx and its helpers are in scope; not a translation unit).  The kernel is
// pt_despeckle.hip's, behind pt_image_launch.hpp; what the calls refuse in their arguments is pt_despeckle_rule.hpp's.
//
// Both calls take historyMerge's path: all submitted work lands, the inputs must render surfaces at the image's size, a group gathers FRAME and
// T on its first stream's context, the records of the current inputs, one launch into the reprojection's scratch (dRpFrame, dRpStats, dRpKept;
// dKappa for scale_out — no buffer of their own).  The read-only call copies the scratch out and touches nothing else; the other one stores it as
// the merge does (storeReprojected: the image keeps its camera, written again, and a group gets its shards back through the host).
extern "C++" {
#include "pt_despeckle_rule.hpp"
}

namespace {
// `store`: pt_despeckle_frame (rgbaOut is null); else pt_despeckle
int despeckleImage(pt_ctx* c, const char* who, const pt_despeckle_rule& r, bool store, float* rgbaOut, float* scaleOut, int64_t* nClamped) {
    const std::string w(who);
    int rc;
    if ((rc = needWholeImage(c, PT_ERR_UNSUPPORTED, who))) return rc;
    if ((rc = syncAll(c))) return rc;                             // work in flight lands in FRAME and T first
    pt_ctx* on = firstStream(c);
    FrameIn cur;
    if ((rc = usableInputs(on, w, "tell apart", cur))) return rc;
    DespeckleJob j;
    if ((rc = wholeFrame(c, PT_ERR_UNSUPPORTED, who, &on, &j.frame))) return rc;      // a group: gathered on on->stream
    if ((rc = wholeStats(c, on, &j.stats))) return rc;
    if (!j.stats && std::isfinite(r.own_z))
        return fail(PT_ERR_ARG, w + ": a finite rule.own_z needs the luminance moments (T was never allocated): call pt_record_moments before rendering, or pass +inf");
    if ((rc = currentRecords(on, nullptr, who))) return rc;
    HIP_TRY(hipSetDevice(on->device));
    const size_t n = (size_t)c->W * c->H;
    HIP_TRY(on->dRpFrame.ensure(n * 16));
    if (store && j.stats) HIP_TRY(on->dRpStats.ensure(n * 16));
    HIP_TRY(on->dRpKept.ensure(8));
    if (scaleOut) HIP_TRY(on->dKappa.ensure(n * 4));
    j.feat = on->rec[ptp::RC_FEAT].recs;
    j.W = c->W; j.H = c->H; j.radius = r.radius; j.minTaps = r.min_taps;
    j.sigmas = r.sigmas; j.ownZ = r.own_z; j.normalTol = r.normal_tol; j.minLum = r.min_lum;
    j.overlay[0] = cur.mouse[0]; j.overlay[1] = cur.mouse[1]; j.overlay[2] = cur.params[2];
    j.mean = !store;
    j.outFrame = on->dRpFrame; j.outStats = store && j.stats ? on->dRpStats.p : nullptr;
    j.scale = scaleOut ? on->dKappa.p : nullptr; j.clamped = on->dRpKept;
    HIP_TRY(despeckleLaunch(j, on->stream));
    if (scaleOut) HIP_TRY(hipMemcpyAsync(scaleOut, on->dKappa, n * 4, hipMemcpyDeviceToHost, on->stream));
    if (store) {
        if ((rc = storeReprojected(c, on, j.stats != nullptr, nClamped))) return rc;  // (records the same camera again)
        HIP_TRY(hipStreamSynchronize(on->stream));
        return 0;
    }
    unsigned cnt = 0;
    if (rgbaOut) HIP_TRY(hipMemcpyAsync(rgbaOut, on->dRpFrame, n * 16, hipMemcpyDeviceToHost, on->stream));
    HIP_TRY(hipMemcpyAsync(&cnt, on->dRpKept, 4, hipMemcpyDeviceToHost, on->stream));
    HIP_TRY(hipStreamSynchronize(on->stream));
    *nClamped = cnt;
    return 0;
}
}  // namespace

int pt_despeckle(pt_ctx* c, const pt_despeckle_rule* rule, float* rgba_out, float* scale_out, int64_t* n_clamped) {
    return counted(n_clamped, [&](int64_t* n) {
        if (int rc = fail(ptp::checkDespeckleRule("pt_despeckle", c, rule))) return rc;
        return despeckleImage(c, "pt_despeckle", *rule, false, rgba_out, scale_out, n);
    });
}

int pt_despeckle_frame(pt_ctx* c, const pt_despeckle_rule* rule, float* scale_out, int64_t* n_clamped) {
    return counted(n_clamped, [&](int64_t* n) {
        if (int rc = fail(ptp::checkDespeckleRule("pt_despeckle_frame", c, rule))) return rc;
        return despeckleImage(c, "pt_despeckle_frame", *rule, true, nullptr, scale_out, n);
    });
}
