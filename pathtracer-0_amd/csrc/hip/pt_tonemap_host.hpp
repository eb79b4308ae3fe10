// pt_tonemap_host.hpp — the host half of pt_tonemap and pt_tonemap_save_png (include/pt_tonemap.h), behind the C ABI (included at the end of
// pt_image.hpp, inside pt_hip.hip's extern "C" block, where pt_ctx and its helpers are in scope; not a translation unit).  The kernels are
// pt_tonemap.hip's, behind pt_image_launch.hpp; what the calls refuse in their arguments, the metered exposure (step 3) and the sRGB threshold
// table are pt_tonemap_rule.hpp's.
//
// Both calls take pt_read_display_mean's path: all submitted work lands, a group gathers FRAME on its first stream's context (wholeFrame), and
// everything runs on that stream.  A given image is uploaded into the reprojection's scratch (dRpFrame); the histogram lives in dRpKept and the
// bytes in dDisplay — no buffer of their own, and nothing of the context is written.  The histogram comes back to the host, step 3 runs there,
// and the second launch takes the exposure as an argument.  The outputs are written last, when nothing can fail any more.
extern "C++" {
#include "pt_tonemap_rule.hpp"
}

namespace {
// the bytes of the rule into rgb (host, W*H*3, may be null), the exposure into *exposure and the histogram into hist (host, may be null)
int tonemapImage(pt_ctx* c, const char* who, const pt_tonemap_rule& r, const float* rgbaIn, float prev, uint8_t* rgb, float* exposure, uint32_t* hist) {
    int rc;
    if ((rc = needWholeImage(c, PT_ERR_UNSUPPORTED, who))) return rc;
    if ((rc = syncAll(c))) return rc;                             // work in flight lands in FRAME first
    pt_ctx* on = firstStream(c);
    TonemapJob j;
    j.perPixel = !rgbaIn;
    if (!rgbaIn) { if ((rc = wholeFrame(c, PT_ERR_UNSUPPORTED, who, &on, &j.image))) return rc; }      // a group: gathered on on->stream
    HIP_TRY(hipSetDevice(on->device));
    const size_t n = (size_t)c->W * c->H;
    if (rgbaIn) {
        HIP_TRY(on->dRpFrame.ensure(n * 16));
        HIP_TRY(hipMemcpyAsync(on->dRpFrame, rgbaIn, n * 16, hipMemcpyHostToDevice, on->stream));
        j.image = on->dRpFrame;
    }
    j.W = c->W; j.H = c->H;
    uint32_t h[PT_TONEMAP_BINS] = {};
    if (hist || !(r.exposure > 0.0f)) {
        HIP_TRY(on->dRpKept.ensure(sizeof h));
        j.hist = on->dRpKept;
        HIP_TRY(tonemapLaunch(j, on->stream));
        HIP_TRY(hipMemcpyAsync(h, on->dRpKept, sizeof h, hipMemcpyDeviceToHost, on->stream));
        HIP_TRY(hipStreamSynchronize(on->stream));
        j.hist = nullptr;
    }
    const float e = ptp::tonemapExposure(h, r, prev);
    if (rgb) {
        HIP_TRY(on->dDisplay.ensure(n * 3));
        j.bytes = on->dDisplay;
        j.exposure = e; j.white = r.white; j.curve = r.curve; j.transfer = r.transfer;
        HIP_TRY(tonemapLaunch(j, on->stream));
        HIP_TRY(hipMemcpyAsync(rgb, on->dDisplay, n * 3, hipMemcpyDeviceToHost, on->stream));
    }
    HIP_TRY(hipStreamSynchronize(on->stream));                    // (also: the upload has left rgbaIn)
    *exposure = e;
    if (hist) std::memcpy(hist, h, sizeof h);
    return 0;
}
}  // namespace

int pt_tonemap(pt_ctx* c, const pt_tonemap_rule* rule, const float* rgba_in, float prev_exposure, uint8_t* rgb_out, float* exposure_out, uint32_t* hist_out) {
    if (int rc = fail(ptp::checkTonemapRule("pt_tonemap", c, rule, prev_exposure))) return rc;
    float e = 0.0f;
    if (int rc = tonemapImage(c, "pt_tonemap", *rule, rgba_in, prev_exposure, rgb_out, &e, hist_out)) return rc;
    if (exposure_out) *exposure_out = e;
    return PT_OK;
}

int pt_tonemap_save_png(pt_ctx* c, const pt_tonemap_rule* rule, const float* rgba_in, float prev_exposure, const char* path, float* exposure_out) {
    if (int rc = fail(ptp::checkTonemapRule("pt_tonemap_save_png", c, rule, prev_exposure))) return rc;
    if (!path) return fail(PT_ERR_ARG, "pt_tonemap_save_png: null argument");
    std::vector<uint8_t> rgb((size_t)c->W * c->H * 3);
    float e = 0.0f;
    if (int rc = tonemapImage(c, "pt_tonemap_save_png", *rule, rgba_in, prev_exposure, rgb.data(), &e, nullptr)) return rc;
    const std::vector<uint8_t> png = encodePng(rgb.data(), c->W, c->H);
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(PT_ERR_ARG, std::string("pt_tonemap_save_png: cannot open ") + path);
    const bool ok = std::fwrite(png.data(), 1, png.size(), f) == png.size();
    if (std::fclose(f) != 0 || !ok) return fail(PT_ERR_ARG, std::string("pt_tonemap_save_png: short write to ") + path);
    if (exposure_out) *exposure_out = e;
    return PT_OK;
}

int pt_tonemap_srgb_thresholds(float out[256]) {
    if (!out) return fail(PT_ERR_ARG, "pt_tonemap_srgb_thresholds: null argument");
    std::memcpy(out, ptp::kTonemapSrgbThresholds, sizeof ptp::kTonemapSrgbThresholds);
    return PT_OK;
}
