// pt_bloom_host.hpp — the host half of pt_bloom, pt_tonemap_bloom and pt_tonemap_bloom_save_png (include/pt_bloom.h), behind the C ABI (included at the
// end of pt_image.hpp, inside pt_hip.hip's extern "C" block, where pt_ctx and its helpers are in scope; not a translation unit).  The kernels are
// pt_bloom.hip's and pt_tonemap.hip's, behind pt_image_launch.hpp; what the calls refuse in their arguments, the level table, norm and T are
// pt_bloom_rule.hpp's and pt_tonemap_rule.hpp's.
//
// The calls take pt_read_display_mean's path: all submitted work lands, a group gathers FRAME on its first stream's context (wholeFrame), and
// everything runs on that stream.  The source is FRAME, a host image uploaded into the reprojection's scratch (dRpFrame, as pt_tonemap's), or the image
// a filter left in dDnOut (on->filteredThere, which pt_image.hpp sets and clears where it writes that buffer): for that one nothing of W*H*16 bytes is
// copied in either direction — the kernels read dDnOut where it lies.  The pyramid (dBloomPyr) and the composed image (dBloomOut, which must not be
// the source) are the context's own, ensured on first use; the histogram lives in dRpKept and the bytes in dDisplay.  Nothing else of the context is
// written.  The outputs are written last, when nothing can fail any more.
extern "C++" {
#include "pt_bloom_rule.hpp"
}

namespace {
// the source image of a bloom call on the device of *on (firstStream(c)), ordered on on->stream: FRAME (perPixel), the upload of rgbaIn, or dDnOut
int bloomSource(pt_ctx* c, const char* who, int source, const float* rgbaIn, pt_ctx** onOut, const float4** image, bool* perPixel) {
    int rc;
    if ((rc = needWholeImage(c, PT_ERR_UNSUPPORTED, who))) return rc;
    pt_ctx* on = firstStream(c);
    if (source == PT_BLOOM_SRC_FILTERED && !on->filteredThere)
        return fail(PT_ERR_ARG, std::string(who) + ": no filtered image on the device (pt_denoise, pt_denoise_guided* or pt_read_display_denoised* first; "
                                                   "pt_select_guided* on an image without luminance moments overwrites it)");
    if ((rc = syncAll(c))) return rc;                             // work in flight lands in FRAME first
    *perPixel = source == PT_BLOOM_SRC_FRAME;
    if (source == PT_BLOOM_SRC_FRAME) { if ((rc = wholeFrame(c, PT_ERR_UNSUPPORTED, who, &on, image))) return rc; }      // a group: gathered on on->stream
    HIP_TRY(hipSetDevice(on->device));
    if (source == PT_BLOOM_SRC_HOST) {
        const size_t bytes = (size_t)c->W * c->H * 16;
        HIP_TRY(on->dRpFrame.ensure(bytes));
        HIP_TRY(hipMemcpyAsync(on->dRpFrame, rgbaIn, bytes, hipMemcpyHostToDevice, on->stream));
        *image = on->dRpFrame;
    }
    if (source == PT_BLOOM_SRC_FILTERED) *image = on->dDnOut;
    *onOut = on;
    return 0;
}

// steps 0-4 of `image` under the exposure e into on->dBloomOut, enqueued on on->stream
int bloomInto(pt_ctx* on, const pt_bloom_rule& b, const float4* image, bool perPixel, float e) {
    BloomJob j;
    j.image = image; j.perPixel = perPixel; j.W = on->W; j.H = on->H; j.levels = b.levels;
    j.T = ptp::bloomThreshold(b.threshold, e); j.spread = b.spread; j.norm = ptp::bloomNorm(b.spread, b.levels); j.intensity = b.intensity;
    HIP_TRY(on->dBloomPyr.ensure(ptp::bloomPyramid(on->W, on->H, PT_BLOOM_MAX_LEVELS).texels * 16));      // sized once, for every level count
    HIP_TRY(on->dBloomOut.ensure((size_t)on->W * on->H * 16));
    j.pyramid = on->dBloomPyr; j.out = on->dBloomOut;
    HIP_TRY(bloomLaunch(j, on->stream));
    return 0;
}

// pt_tonemap_bloom's chain: the bytes into rgb (host, W*H*3, may be null), the exposure into *exposure and the histogram into hist (host, may be null)
int tonemapBloomImage(pt_ctx* c, const char* who, const pt_tonemap_rule& r, const pt_bloom_rule& b, int source, const float* rgbaIn, float prev, uint8_t* rgb,
                      float* exposure, uint32_t* hist) {
    pt_ctx* on = nullptr;
    TonemapJob j;
    if (int rc = bloomSource(c, who, source, rgbaIn, &on, &j.image, &j.perPixel)) return rc;
    const size_t n = (size_t)c->W * c->H;
    j.W = c->W; j.H = c->H;
    uint32_t h[PT_TONEMAP_BINS] = {};
    if (hist || !(r.exposure > 0.0f)) {                           // pt_tonemap's steps 1-3, on the source image
        HIP_TRY(on->dRpKept.ensure(sizeof h));
        j.hist = on->dRpKept;
        HIP_TRY(tonemapLaunch(j, on->stream));
        HIP_TRY(hipMemcpyAsync(h, on->dRpKept, sizeof h, hipMemcpyDeviceToHost, on->stream));
        HIP_TRY(hipStreamSynchronize(on->stream));
        j.hist = nullptr;
    }
    const float e = ptp::tonemapExposure(h, r, prev);
    if (rgb) {
        if (int rc = bloomInto(on, b, j.image, j.perPixel, e)) return rc;
        HIP_TRY(on->dDisplay.ensure(n * 3));
        j.image = on->dBloomOut; j.perPixel = false;              // the composed image is a mean already: steps 4-5 as they are
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

// the argument checks of the two display calls: pt_tonemap's, then the bloom's
int checkTonemapBloom(const char* who, pt_ctx* c, const pt_tonemap_rule* rule, const pt_bloom_rule* bloom, int source, const float* rgbaIn, float prev) {
    if (int rc = fail(ptp::checkTonemapRule(who, c, rule, prev))) return rc;
    return fail(ptp::checkBloomRule(who, c, bloom, source, rgbaIn, nullptr));
}
}  // namespace

int pt_bloom(pt_ctx* c, const pt_bloom_rule* rule, int source, const float* rgba_in, float exposure, float* rgba_out) {
    if (int rc = fail(ptp::checkBloomRule("pt_bloom", c, rule, source, rgba_in, &exposure))) return rc;
    pt_ctx* on = nullptr; const float4* image = nullptr; bool perPixel = false;
    if (int rc = bloomSource(c, "pt_bloom", source, rgba_in, &on, &image, &perPixel)) return rc;
    if (int rc = bloomInto(on, *rule, image, perPixel, exposure)) return rc;
    if (rgba_out) HIP_TRY(hipMemcpyAsync(rgba_out, on->dBloomOut, (size_t)c->W * c->H * 16, hipMemcpyDeviceToHost, on->stream));
    HIP_TRY(hipStreamSynchronize(on->stream));
    return PT_OK;
}

int pt_tonemap_bloom(pt_ctx* c, const pt_tonemap_rule* rule, const pt_bloom_rule* bloom, int source, const float* rgba_in, float prev_exposure, uint8_t* rgb_out,
                     float* exposure_out, uint32_t* hist_out) {
    if (int rc = checkTonemapBloom("pt_tonemap_bloom", c, rule, bloom, source, rgba_in, prev_exposure)) return rc;
    float e = 0.0f;
    if (int rc = tonemapBloomImage(c, "pt_tonemap_bloom", *rule, *bloom, source, rgba_in, prev_exposure, rgb_out, &e, hist_out)) return rc;
    if (exposure_out) *exposure_out = e;
    return PT_OK;
}

int pt_tonemap_bloom_save_png(pt_ctx* c, const pt_tonemap_rule* rule, const pt_bloom_rule* bloom, int source, const float* rgba_in, float prev_exposure,
                              const char* path, float* exposure_out) {
    if (int rc = checkTonemapBloom("pt_tonemap_bloom_save_png", c, rule, bloom, source, rgba_in, prev_exposure)) return rc;
    if (!path) return fail(PT_ERR_ARG, "pt_tonemap_bloom_save_png: null argument");
    std::vector<uint8_t> rgb((size_t)c->W * c->H * 3);
    float e = 0.0f;
    if (int rc = tonemapBloomImage(c, "pt_tonemap_bloom_save_png", *rule, *bloom, source, rgba_in, prev_exposure, rgb.data(), &e, nullptr)) return rc;
    const std::vector<uint8_t> png = encodePng(rgb.data(), c->W, c->H);
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(PT_ERR_ARG, std::string("pt_tonemap_bloom_save_png: cannot open ") + path);
    const bool ok = std::fwrite(png.data(), 1, png.size(), f) == png.size();
    if (std::fclose(f) != 0 || !ok) return fail(PT_ERR_ARG, std::string("pt_tonemap_bloom_save_png: short write to ") + path);
    if (exposure_out) *exposure_out = e;
    return PT_OK;
}
