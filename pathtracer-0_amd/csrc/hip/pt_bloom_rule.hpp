// pt_bloom_rule.hpp — the host-only part of pt_bloom, pt_tonemap_bloom and pt_tonemap_bloom_save_png (include/pt_bloom.h): what they refuse in
// their bloom arguments before their first HIP call (the null checks, the rule's fields in the struct's order, the source, the image that must fit
// it, then pt_bloom's exposure; the first failing one as a code and a text that carries the calling entry point's name), the sizes and offsets of the
// pyramid's levels, and the two numbers the host computes for the kernels: norm (step 3) and T (step 1).  Plain C++: no HIP runtime call and no
// context, so tests/c/bloom_rule_check.cpp runs all of it on a CPU.
//
// The refusals that read the context (a whole image, a filtered image that is there) are not here: they follow in pt_bloom_host.hpp.  The tone-map
// rule of pt_tonemap_bloom is pt_tonemap_rule.hpp's to check.
#pragma once
#include "../../../include/pt_bloom.h"
#include "pt_image_history.hpp"      // ptp::Refused

#include <cmath>
#include <cstddef>
#include <string>

namespace ptp {

// every check below, in the order it is made (the test requires each of them of its grid)
enum BloomCheck { BC_OK, BC_CTX, BC_RULE, BC_LEVELS, BC_INTENSITY, BC_THRESHOLD, BC_SPREAD, BC_SOURCE, BC_IMAGE, BC_EXPOSURE, BC_COUNT };

// the first check that fails: which = its BloomCheck (may be null).  exposure: pt_bloom's, or null for the calls that meter their own
inline Refused checkBloomRule(const char* who, const void* ctx, const pt_bloom_rule* r, int source, const void* rgbaIn, const float* exposure, int* which = nullptr) {
    const std::string w = std::string(who) + ": ";
    auto refuse = [&](BloomCheck k, const std::string& text) { if (which) *which = k; return Refused{PT_ERR_ARG, w + text}; };
    if (which) *which = BC_OK;
    if (!ctx) return refuse(BC_CTX, "null context");
    if (!r) return refuse(BC_RULE, "null bloom rule");
    if (r->levels < 1 || r->levels > PT_BLOOM_MAX_LEVELS) return refuse(BC_LEVELS, "bloom.levels must lie in 1 .. 8");
    if (!(std::isfinite(r->intensity) && r->intensity >= 0.0f)) return refuse(BC_INTENSITY, "bloom.intensity must be finite and >= 0");
    if (!(std::isfinite(r->threshold) && r->threshold >= 0.0f)) return refuse(BC_THRESHOLD, "bloom.threshold must be finite and >= 0");
    if (!(r->spread > 0.0f && r->spread <= 1.0f)) return refuse(BC_SPREAD, "bloom.spread must lie in (0, 1]");
    if (source != PT_BLOOM_SRC_FRAME && source != PT_BLOOM_SRC_HOST && source != PT_BLOOM_SRC_FILTERED)
        return refuse(BC_SOURCE, "source must be PT_BLOOM_SRC_FRAME, PT_BLOOM_SRC_HOST or PT_BLOOM_SRC_FILTERED");
    if ((source == PT_BLOOM_SRC_HOST) != (rgbaIn != nullptr))
        return refuse(BC_IMAGE, source == PT_BLOOM_SRC_HOST ? "PT_BLOOM_SRC_HOST needs rgba_in" : "rgba_in must be NULL unless the source is PT_BLOOM_SRC_HOST");
    if (exposure && !(std::isfinite(*exposure) && *exposure > 0.0f)) return refuse(BC_EXPOSURE, "exposure must be finite and > 0");
    return {};
}

// The pyramid of a W x H image under `levels` levels: level[0] is the source (not stored: offset 0 means nothing there), level[k], k = 1 .. levels,
// lies at `offset` texels (float4) of one allocation of `texels` texels
struct BloomLevel { int W, H; size_t offset; };
struct BloomPyramid { int levels; BloomLevel level[PT_BLOOM_MAX_LEVELS + 1]; size_t texels; };
inline BloomPyramid bloomPyramid(int W, int H, int levels) {
    BloomPyramid p{};
    p.levels = levels;
    p.level[0] = {W, H, 0};
    for (int k = 1; k <= levels; k++) {
        p.level[k] = {(p.level[k - 1].W + 1) / 2, (p.level[k - 1].H + 1) / 2, p.texels};
        p.texels += (size_t)p.level[k].W * p.level[k].H;
    }
    return p;
}

// norm of step 3, in the header's order
inline float bloomNorm(float spread, int levels) {
    float p = 1.0f, sum = 1.0f;
    for (int k = 1; k < levels; k++) { p = p * spread; sum = sum + p; }
    return 1.0f / sum;
}
// T of step 1
inline float bloomThreshold(float threshold, float exposure) { return threshold / exposure; }

}  // namespace ptp
