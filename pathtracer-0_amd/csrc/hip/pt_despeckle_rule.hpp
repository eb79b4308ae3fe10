// pt_despeckle_rule.hpp — what pt_despeckle and pt_despeckle_frame (include/pt_despeckle.h) refuse in their arguments, before their first HIP call:
// the null checks, then the rule's fields in the struct's order, the first failing one as a code and a text that carries the calling entry point's
// name.  Plain C++: no HIP runtime call and no context, so tests/c/despeckle_rule_check.cpp runs every refusal on a CPU.  (The table of
// pt_image_args.hpp holds the calls that existed when it was written, row for row; these two have one rule and one order and need no row.)
//
// The refusals that read the context (a whole image, Parameters or ORIGIN not set, DEBUG != 0, own_z finite without T) are not here: they follow
// the argument checks in pt_despeckle_host.hpp.
#pragma once
#include "../../../include/pt_despeckle.h"
#include "pt_image_history.hpp"      // ptp::Refused

#include <cmath>
#include <string>

namespace ptp {

// every check below, in the order it is made (the test requires each of them of its grid)
enum DespeckleCheck { DC_OK, DC_CTX, DC_RULE, DC_RADIUS, DC_SIGMAS, DC_MIN_TAPS, DC_OWN_Z, DC_NORMAL_TOL, DC_MIN_LUM, DC_COUNT };

// the largest min_taps of a radius: the window without its centre
inline int despeckleWindowTaps(int radius) { return (2 * radius + 1) * (2 * radius + 1) - 1; }

// the first check that fails: which = its DespeckleCheck (may be null)
inline Refused checkDespeckleRule(const char* who, const void* ctx, const pt_despeckle_rule* r, int* which = nullptr) {
    const std::string w = std::string(who) + ": ";
    auto refuse = [&](DespeckleCheck k, const std::string& text) { if (which) *which = k; return Refused{PT_ERR_ARG, w + text}; };
    if (which) *which = DC_OK;
    if (!ctx) return refuse(DC_CTX, "null context");
    if (!r) return refuse(DC_RULE, "null rule");
    if (r->radius < 1 || r->radius > 3) return refuse(DC_RADIUS, "rule.radius must be 1 .. 3");
    if (!(std::isfinite(r->sigmas) && r->sigmas >= 0.0f)) return refuse(DC_SIGMAS, "rule.sigmas must be finite and >= 0");
    if (r->min_taps < 2 || r->min_taps > despeckleWindowTaps(r->radius))
        return refuse(DC_MIN_TAPS, "rule.min_taps must be 2 .. (2*radius + 1)^2 - 1 = " + std::to_string(despeckleWindowTaps(r->radius)));
    if (!(r->own_z > 0.0f)) return refuse(DC_OWN_Z, "rule.own_z must be > 0 (+inf turns the test off)");
    if (!(r->normal_tol >= -1.0f && r->normal_tol <= 1.0f)) return refuse(DC_NORMAL_TOL, "rule.normal_tol must lie in [-1, 1]");
    if (!(std::isfinite(r->min_lum) && r->min_lum >= 0.0f)) return refuse(DC_MIN_LUM, "rule.min_lum must be finite and >= 0");
    return {};
}

}  // namespace ptp
