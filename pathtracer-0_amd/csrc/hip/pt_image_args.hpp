// pt_image_args.hpp — what every image-space call of the C ABI refuses in its arguments, before its first HIP call: one enumerator per entry point,
// one struct for whatever they can be given, each predicate and its refusal text once, and one table row per entry point with the checks it makes
// in the order it makes them (an entry point that makes another's checks under its own name asks with that row and its name).  Plain C++: no HIP runtime call and no context.  pt_image.hpp's wrappers (and pt_render_adaptive in pt_hip.hip) fill
// the struct and ask checkImageArgs; tests/c/image_args_check.cpp asks the same from scripts, so every refusal can be run on a CPU.
//
// The refusals that read the context (a whole image, moments never allocated, Parameters or ORIGIN not set, DEBUG != 0, more than 4096 materials
// under PT_THROUGH_KEY, whatever ImageHistory answers) are not here: they follow the argument checks where they always did.
//
// THE ROWS HOLD THE ABI AS IT GREW, not as one would design it: the four pt_denoise_guided* calls answer range errors as
// "pt_denoise_guided:", pt_reproject_frame_demod as "pt_reproject_frame:" but its floor under its own name; the two demodulated steering calls look at
// the floor before the null pointers; the fill calls check sigma from the second entry on and neither iterations nor min_frames; a rule's sigma
// comes before its min_frames, a call's own after it; pt_reproject_frame_moved takes a floor of 0 and pt_reproject_frame_demod does not.
#pragma once
#include "../../../include/pt_reproject.h"
#include "../../../include/pt_steer.h"
#include "../../../include/pt_through.h"
#include "../../../include/pt_validate.h"
#include "pt_image_history.hpp"      // ptp::Refused

#include <climits>
#include <cstddef>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

// the highest iteration count the filters take (the test builds the table once with another value)
#ifndef PT_ARGS_ITERATIONS_MAX
#define PT_ARGS_ITERATIONS_MAX 8
#endif

namespace ptp {

enum ImageCall {
    IC_RECORD_MOMENTS, IC_READ_MOMENTS, IC_WRITE_MOMENTS, IC_READ_FEATURES, IC_DENOISE, IC_READ_DISPLAY_DENOISED, IC_DENOISE_GUIDED,
    IC_READ_DISPLAY_DENOISED_GUIDED, IC_DENOISE_GUIDED_DEMOD, IC_READ_DISPLAY_DENOISED_GUIDED_DEMOD, IC_REPROJECT_FRAME, IC_REPROJECT_FRAME_DEMOD,
    IC_REPROJECT_FRAME_THROUGH, IC_REPROJECT_FRAME_BILINEAR, IC_MOTION_MARK, IC_REPROJECT_FRAME_MOVED, IC_HISTORY_HOLD, IC_HISTORY_MERGE, IC_RENDER_MASK,
    IC_SELECT_GUIDED, IC_RENDER_ADAPTIVE_GUIDED, IC_SELECT_GUIDED_DEMOD, IC_RENDER_ADAPTIVE_GUIDED_DEMOD, IC_RENDER_INTERLEAVED, IC_FILL_FRAME,
    IC_DENOISE_GUIDED_FILLED, IC_READ_DISPLAY_DENOISED_GUIDED_FILLED, IC_READ_FEATURES_THROUGH, IC_READ_THROUGH_RAYS, IC_FILL_FRAME_THROUGH,
    IC_DENOISE_GUIDED_THROUGH, IC_READ_DISPLAY_DENOISED_GUIDED_THROUGH, IC_RENDER_ADAPTIVE, IC_COUNT
};

// the pointers a call takes: the context; the image, records or mask it reads or writes; its rule (guided, validate, reprojection); a seen-through
// rule; the seeds; pt_render_mask's mask.  Count outputs may always be null and are not here.
enum ArgPointer { AP_CTX = 1, AP_BUFFER = 2, AP_RULE = 4, AP_THRU = 8, AP_SEEDS = 16, AP_MASK = 32 };

// What any of the calls can be given.  A wrapper fills what its call takes; the rest is never looked at by its row.
struct ImageArgs {
    unsigned present = 0;                                         // ArgPointer bits
    int iterations = 0; float sigma[4] = {}; int min_frames = 0; float albedo_floor = 0;
    pt_through_rule thru{}; pt_guided_rule guided{}; pt_validate_rule validate{};
    float max_history = 0, depth_tol = 0, normal_tol = 0; int flags = 0; float point_tol = 0; int radius = 0; float snap = 0;
    int n_frames = 0, stride = 0, phase_x = 0, phase_y = 0;
    float rel_err = 0, abs_err = 0; int max_frames = 0;

    ImageArgs& has(ArgPointer p, const void* v) { if (v) present |= p; return *this; }
    // a call's context, and the image, records or mask it reads or writes
    static ImageArgs given(const void* ctx, const void* buffer = nullptr) { return ImageArgs().has(AP_CTX, ctx).has(AP_BUFFER, buffer); }
    // a rule behind a pointer: present and copied, or absent
    ImageArgs& has(const pt_through_rule* r) { if (r) thru = *r; return has(AP_THRU, r); }
    ImageArgs& has(const pt_guided_rule* r) { if (r) guided = *r; return has(AP_RULE, r); }
    ImageArgs& has(const pt_validate_rule* r) { if (r) validate = *r; return has(AP_RULE, r); }
    ImageArgs& filter(int it, float s0, float s1, float s2, float s3, int minFrames, float floorA) {
        iterations = it; sigma[0] = s0; sigma[1] = s1; sigma[2] = s2; sigma[3] = s3; min_frames = minFrames; albedo_floor = floorA;
        return *this;
    }
    ImageArgs& floor(float floorA) { albedo_floor = floorA; return *this; }
    ImageArgs& seeded(const void* seeds, int nFrames) { n_frames = nFrames; return has(AP_SEEDS, seeds); }
    ImageArgs& lattice(int s, int px, int py) { stride = s; phase_x = px; phase_y = py; return *this; }
    ImageArgs& adaptive(float relErr, float absErr, int minFrames, int maxFrames) { rel_err = relErr; abs_err = absErr; min_frames = minFrames; max_frames = maxFrames; return *this; }
    ImageArgs& reproject(float maxHistory, float depthTol, float normalTol, int fl, float floorA) {
        max_history = maxHistory; depth_tol = depthTol; normal_tol = normalTol; flags = fl; albedo_floor = floorA;
        return *this;
    }
};

// ---- the fields a check can name: X(enumerator, script name, type, member).  Fields one predicate covers together are adjacent.
#define PT_IMAGE_ARG_FIELDS(X)                                                                                                                     \
    X(AF_ITERATIONS, "iterations", int, iterations) X(AF_SIGMA, "sigma0", float, sigma[0]) X(AF_SIGMA1, "sigma1", float, sigma[1])                 \
    X(AF_SIGMA2, "sigma2", float, sigma[2]) X(AF_SIGMA3, "sigma3", float, sigma[3]) X(AF_MIN_FRAMES, "min_frames", int, min_frames)                \
    X(AF_ALBEDO_FLOOR, "albedo_floor", float, albedo_floor) X(AF_THRU_MAX_DEPTH, "thru.max_depth", int, thru.max_depth)                            \
    X(AF_THRU_MIN_WEIGHT, "thru.min_weight", float, thru.min_weight) X(AF_THRU_LOBES, "thru.lobes", int, thru.lobes)                               \
    X(AF_THRU_FLAGS, "thru.flags", int, thru.flags) X(AF_RULE_ITERATIONS, "guided.iterations", int, guided.iterations)                             \
    X(AF_RULE_SIGMA, "guided.sigma_lum", float, guided.sigma_lum) X(AF_RULE_SIGMA1, "guided.sigma_normal", float, guided.sigma_normal)             \
    X(AF_RULE_SIGMA2, "guided.sigma_depth", float, guided.sigma_depth) X(AF_RULE_SIGMA3, "guided.sigma_albedo", float, guided.sigma_albedo)        \
    X(AF_RULE_MIN_FRAMES, "guided.min_frames", int, guided.min_frames) X(AF_RULE_REL_ERR, "guided.rel_err", float, guided.rel_err)                 \
    X(AF_RULE_ABS_ERR, "guided.abs_err", float, guided.abs_err) X(AF_RULE_MAX_FRAMES, "guided.max_frames", int, guided.max_frames)                 \
    X(AF_VAL_RADIUS, "validate.radius", int, validate.radius) X(AF_VAL_Z_LO, "validate.z_lo", float, validate.z_lo)                                \
    X(AF_VAL_Z_HI, "validate.z_hi", float, validate.z_hi) X(AF_VAL_NORMAL_TOL, "validate.normal_tol", float, validate.normal_tol)                  \
    X(AF_MAX_HISTORY, "max_history", float, max_history) X(AF_DEPTH_TOL, "depth_tol", float, depth_tol) X(AF_NORMAL_TOL, "normal_tol", float, normal_tol) \
    X(AF_FLAGS, "flags", int, flags) X(AF_POINT_TOL, "point_tol", float, point_tol) X(AF_RADIUS, "radius", int, radius) X(AF_SNAP, "snap", float, snap) \
    X(AF_N_FRAMES, "n_frames", int, n_frames) X(AF_STRIDE, "stride", int, stride) X(AF_PHASE_X, "phase_x", int, phase_x)                           \
    X(AF_PHASE_Y, "phase_y", int, phase_y) X(AF_REL_ERR, "rel_err", float, rel_err) X(AF_ABS_ERR, "abs_err", float, abs_err)                       \
    X(AF_MAX_FRAMES, "max_frames", int, max_frames)

enum ArgFieldId {
#define X(id, name, type, member) id,
    PT_IMAGE_ARG_FIELDS(X)
#undef X
    AF_COUNT
};
struct ArgField { const char* name; bool isFloat; size_t offset; };
inline bool isFloatField(const int*) { return false; }
inline bool isFloatField(const float*) { return true; }
inline const ArgField& argField(int id) {
    static const ArgField F[AF_COUNT] = {
#define X(id, name, type, member) {name, isFloatField((const type*)nullptr), offsetof(ImageArgs, member)},
        PT_IMAGE_ARG_FIELDS(X)
#undef X
    };
    return F[id];
}
inline int intArg(const ImageArgs& a, int id) { int v; std::memcpy(&v, (const char*)&a + argField(id).offset, 4); return v; }
inline float floatArg(const ImageArgs& a, int id) { float v; std::memcpy(&v, (const char*)&a + argField(id).offset, 4); return v; }

// ---- the predicates.  Of a float interval either end is open or closed; a NaN lies in none.
enum ArgPredicate {
    PR_PRESENT,         // every pointer of `mask`
    PR_INT_RANGE,       // ilo <= field <= ihi (ihi == INT_MAX: "at least")
    PR_INTERVAL,        // each of `n` adjacent float fields within lo .. hi
    PR_ORDERED,         // two adjacent float fields, finite with 0 <= first < second
    PR_FLAGS,           // no bit outside `mask`
    PR_PHASE,           // two adjacent int fields in [0, stride)
    PR_KEYED            // a seen-through rule that follows chains has PT_THROUGH_KEY
};
struct ArgCheck {
    ArgPredicate pred; int field; int n; unsigned mask; int ilo, ihi; float lo, hi; bool loOpen, hiOpen;
    const char* label;      // how the message names what it looked at: data, since "iterations" here is "rule.iterations" there
    const char* tail;       // PR_INTERVAL: the wording of its bounds
    const char* note;       // in parentheses behind the message, or ""
    bool own;               // the message carries the call's own name where the row's prefix is another call's
};

inline bool holds(const ArgCheck& k, const ImageArgs& a) {
    switch (k.pred) {
        case PR_PRESENT: return (a.present & k.mask) == k.mask;
        case PR_INT_RANGE: { const int v = intArg(a, k.field); return v >= k.ilo && v <= k.ihi; }
        case PR_INTERVAL:
            for (int i = 0; i < k.n; i++) {
                const float v = floatArg(a, k.field + i);
                if (!((k.loOpen ? v > k.lo : v >= k.lo) && (k.hiOpen ? v < k.hi : v <= k.hi))) return false;
            }
            return true;
        case PR_ORDERED: {
            const float lo = floatArg(a, k.field), hi = floatArg(a, k.field + 1);
            return __builtin_isfinite(lo) && __builtin_isfinite(hi) && lo >= 0.0f && lo < hi;
        }
        case PR_FLAGS: return !(intArg(a, k.field) & ~(int)k.mask);
        case PR_PHASE: {
            const int x = intArg(a, k.field), y = intArg(a, k.field + 1);
            return x >= 0 && x < a.stride && y >= 0 && y < a.stride;
        }
        case PR_KEYED: return !(a.thru.max_depth > 0 && a.thru.lobes != 0 && !(a.thru.flags & PT_THROUGH_KEY));
    }
    return false;
}
inline std::string refusalText(const ArgCheck& k) {
    const std::string l(k.label);
    switch (k.pred) {
        case PR_PRESENT: return "null " + l;
        case PR_INT_RANGE:
            if (k.ihi == INT_MAX) return l + " must be >= " + std::to_string(k.ilo) + k.note;
            return l + " must be in [" + std::to_string(k.ilo) + "," + std::to_string(k.ihi) + "]";
        case PR_INTERVAL: return l + k.tail + k.note;
        case PR_ORDERED: return l + " must be finite with 0 <= z_lo < z_hi";
        case PR_FLAGS: return "unknown " + l;
        case PR_PHASE: return "a phase must be in [0, stride)";
        case PR_KEYED: return "a rule that follows chains needs PT_THROUGH_KEY (the surface word is what a source is matched on)";
    }
    return l;
}

// ---- the checks a row can list
namespace args {
using List = std::vector<ArgCheck>;
constexpr float INF = std::numeric_limits<float>::infinity();
inline ArgCheck make(ArgPredicate p, int field, const char* label) { return ArgCheck{p, field, 1, 0u, 0, 0, 0.0f, 0.0f, false, false, label, "", "", false}; }
inline ArgCheck present(unsigned mask, const char* what) { ArgCheck k = make(PR_PRESENT, -1, what); k.mask = mask; k.own = true; return k; }
inline ArgCheck intRange(int field, int lo, int hi, const char* label, const char* note = "") {
    ArgCheck k = make(PR_INT_RANGE, field, label); k.ilo = lo; k.ihi = hi; k.note = note; return k;
}
inline ArgCheck atLeast(int field, int lo, const char* label, const char* note = "") { return intRange(field, lo, INT_MAX, label, note); }
inline ArgCheck interval(int field, int n, float lo, bool loOpen, float hi, bool hiOpen, const char* label, const char* tail, const char* note = "") {
    ArgCheck k = make(PR_INTERVAL, field, label); k.n = n; k.lo = lo; k.loOpen = loOpen; k.hi = hi; k.hiOpen = hiOpen; k.tail = tail; k.note = note; return k;
}
// > 0 and not NaN; >= 0 and not NaN; finite and > 0; 0 or finite and > 0 (-0.0 is 0)
inline ArgCheck positive(int field, int n, const char* label, const char* note = "") { return interval(field, n, 0.0f, true, INF, false, label, " must be > 0", note); }
inline ArgCheck notNegative(int field, int n, const char* label) { return interval(field, n, 0.0f, false, INF, false, label, " must be >= 0 and not NaN"); }
inline ArgCheck finitePositive(int field, const char* label, bool own) {
    ArgCheck k = interval(field, 1, 0.0f, true, INF, true, label, " must be finite and > 0"); k.own = own; return k;
}
inline ArgCheck zeroOrFinitePositive(int field, const char* label) { return interval(field, 1, 0.0f, false, INF, true, label, " must be 0 or finite and > 0"); }
inline ArgCheck cosine(int field, const char* label) { return interval(field, 1, -1.0f, false, 1.0f, false, label, " must be in [-1, 1]"); }
inline ArgCheck ordered(int field, const char* label) { ArgCheck k = make(PR_ORDERED, field, label); k.n = 2; return k; }
inline ArgCheck flagsWithin(int field, unsigned mask, const char* label) { ArgCheck k = make(PR_FLAGS, field, label); k.mask = mask; return k; }
inline ArgCheck phase(int field) { ArgCheck k = make(PR_PHASE, field, "a phase"); k.n = 2; return k; }
inline ArgCheck keyed() { return make(PR_KEYED, AF_THRU_FLAGS, "rule.flags"); }
inline List operator+(List a, const List& b) { a.insert(a.end(), b.begin(), b.end()); return a; }
}  // namespace args

struct ImageCallRow { ImageCall call; const char* name; const char* prefix; std::vector<ArgCheck> checks; };

// ---- THE TABLE: per entry point its name, the prefix of its messages (of all but the checks marked `own`), and its checks in their order
inline const std::vector<ImageCallRow>& imageCallTable() {
    using namespace args;
    static const std::vector<ImageCallRow> T = [] {
        const char* const OFF = " (+inf switches its term off)";
        const char* const NO_CAP = " (0 = no cap)";
        const List ctx{present(AP_CTX, "context")};
        const auto given = [](unsigned mask) { return List{present(AP_CTX | mask, "argument")}; };
        const List nFrames{atLeast(AF_N_FRAMES, 1, "n_frames")};
        const List iterations{intRange(AF_ITERATIONS, 0, PT_ARGS_ITERATIONS_MAX, "iterations")};
        const List minFrames{atLeast(AF_MIN_FRAMES, 2, "min_frames")};
        const auto sigmaFrom = [OFF](int first) { return List{positive(AF_SIGMA + first, 4 - first, "every sigma", OFF)}; };
        const List atrous = iterations + sigmaFrom(0);                        // pt_denoise
        const List filter = iterations + minFrames + sigmaFrom(0);            // the guided filter
        const List fill = sigmaFrom(1);                                       // the prefill alone: no luminance term, no iterations, no min_frames
        const List floorOwn{finitePositive(AF_ALBEDO_FLOOR, "albedo_floor", true)};
        const List floorOr0{zeroOrFinitePositive(AF_ALBEDO_FLOOR, "albedo_floor")};
        const List thru{present(AP_THRU, "rule"), intRange(AF_THRU_MAX_DEPTH, 0, 8, "rule.max_depth"),
                        interval(AF_THRU_MIN_WEIGHT, 1, 0.0f, true, 1.0f, false, "rule.min_weight", " must be in (0,1]"), intRange(AF_THRU_LOBES, 0, 3, "rule.lobes"),
                        flagsWithin(AF_THRU_FLAGS, PT_THROUGH_KEY, "rule.flags")};
        const List guided{intRange(AF_RULE_ITERATIONS, 0, 8, "rule.iterations"), positive(AF_RULE_SIGMA, 4, "every sigma of the rule", OFF),
                          atLeast(AF_RULE_MIN_FRAMES, 2, "rule.min_frames"), notNegative(AF_RULE_REL_ERR, 2, "rule.rel_err and rule.abs_err"),
                          atLeast(AF_RULE_MAX_FRAMES, 0, "rule.max_frames", NO_CAP)};
        const List reproject{interval(AF_MAX_HISTORY, 1, 1.0f, false, INF, false, "max_history", " must be >= 1"), positive(AF_DEPTH_TOL, 1, "depth_tol"),
                             cosine(AF_NORMAL_TOL, "normal_tol"), flagsWithin(AF_FLAGS, PT_REPROJECT_ALL_MATERIALS, "flags")};
        const char* const G = "pt_denoise_guided";
        const char* const R = "pt_reproject_frame";
        const auto row = [](ImageCall call, const char* name, const List& checks, const char* prefix = nullptr) {
            return ImageCallRow{call, name, prefix ? prefix : name, checks};
        };
        return std::vector<ImageCallRow>{
            row(IC_RECORD_MOMENTS, "pt_record_moments", ctx),
            row(IC_READ_MOMENTS, "pt_read_moments", given(AP_BUFFER)),
            row(IC_WRITE_MOMENTS, "pt_write_moments", given(AP_BUFFER)),
            row(IC_READ_FEATURES, "pt_read_features", given(AP_BUFFER)),
            row(IC_DENOISE, "pt_denoise", given(AP_BUFFER) + atrous),
            row(IC_READ_DISPLAY_DENOISED, "pt_read_display_denoised", given(AP_BUFFER) + atrous, "pt_denoise"),
            row(IC_DENOISE_GUIDED, G, given(AP_BUFFER) + filter),
            row(IC_READ_DISPLAY_DENOISED_GUIDED, "pt_read_display_denoised_guided", given(AP_BUFFER) + filter, G),
            row(IC_DENOISE_GUIDED_DEMOD, "pt_denoise_guided_demod", given(AP_BUFFER) + floorOwn + filter, G),
            row(IC_READ_DISPLAY_DENOISED_GUIDED_DEMOD, "pt_read_display_denoised_guided_demod", given(AP_BUFFER) + floorOwn + filter, G),
            row(IC_REPROJECT_FRAME, R, ctx + reproject),
            row(IC_REPROJECT_FRAME_DEMOD, "pt_reproject_frame_demod", ctx + floorOwn + reproject, R),
            row(IC_REPROJECT_FRAME_THROUGH, "pt_reproject_frame_through",
                given(AP_RULE) + List{intRange(AF_RADIUS, 0, 4, "rule.radius"), positive(AF_POINT_TOL, 1, "rule.point_tol")} + thru + List{keyed()} + reproject),
            row(IC_REPROJECT_FRAME_BILINEAR, "pt_reproject_frame_bilinear",
                given(AP_RULE) + List{interval(AF_SNAP, 1, 0.0f, false, 0.5f, true, "rule.snap", " must be in [0, 0.5)"),
                                      zeroOrFinitePositive(AF_ALBEDO_FLOOR, "rule.albedo_floor")} + reproject),
            row(IC_MOTION_MARK, "pt_motion_mark", ctx),
            row(IC_REPROJECT_FRAME_MOVED, "pt_reproject_frame_moved", ctx + reproject + floorOr0),
            row(IC_HISTORY_HOLD, "pt_history_hold", ctx),
            row(IC_HISTORY_MERGE, "pt_history_merge",
                given(AP_RULE) + List{intRange(AF_VAL_RADIUS, 1, 4, "rule.radius"), ordered(AF_VAL_Z_LO, "rule.z_lo and rule.z_hi"),
                                      cosine(AF_VAL_NORMAL_TOL, "rule.normal_tol")}),
            row(IC_RENDER_MASK, "pt_render_mask", given(AP_SEEDS | AP_MASK) + nFrames),
            row(IC_SELECT_GUIDED, "pt_select_guided", given(AP_RULE | AP_BUFFER) + guided),
            row(IC_RENDER_ADAPTIVE_GUIDED, "pt_render_adaptive_guided", given(AP_SEEDS | AP_RULE) + nFrames + guided),
            row(IC_SELECT_GUIDED_DEMOD, "pt_select_guided_demod", floorOwn + given(AP_RULE | AP_BUFFER) + guided),
            row(IC_RENDER_ADAPTIVE_GUIDED_DEMOD, "pt_render_adaptive_guided_demod", floorOwn + given(AP_SEEDS | AP_RULE) + nFrames + guided),
            row(IC_RENDER_INTERLEAVED, "pt_render_interleaved", given(AP_SEEDS) + nFrames + List{intRange(AF_STRIDE, 1, 8, "stride"), phase(AF_PHASE_X)}),
            row(IC_FILL_FRAME, "pt_fill_frame", given(AP_BUFFER) + floorOr0 + fill),
            row(IC_DENOISE_GUIDED_FILLED, "pt_denoise_guided_filled", given(AP_BUFFER) + floorOr0 + filter),
            row(IC_READ_DISPLAY_DENOISED_GUIDED_FILLED, "pt_read_display_denoised_guided_filled", given(AP_BUFFER) + floorOr0 + filter),
            row(IC_READ_FEATURES_THROUGH, "pt_read_features_through", given(AP_BUFFER) + thru),
            row(IC_READ_THROUGH_RAYS, "pt_read_through_rays", given(AP_BUFFER) + thru),
            row(IC_FILL_FRAME_THROUGH, "pt_fill_frame_through", given(AP_BUFFER) + thru + floorOr0 + fill),
            row(IC_DENOISE_GUIDED_THROUGH, "pt_denoise_guided_through", given(AP_BUFFER) + thru + floorOr0 + filter),
            row(IC_READ_DISPLAY_DENOISED_GUIDED_THROUGH, "pt_read_display_denoised_guided_through", given(AP_BUFFER) + thru + floorOr0 + filter),
            row(IC_RENDER_ADAPTIVE, "pt_render_adaptive",
                given(AP_SEEDS) + nFrames + List{atLeast(AF_MIN_FRAMES, 2, "min_frames", " (a variance needs two frames)"),
                                                 atLeast(AF_MAX_FRAMES, 0, "max_frames", NO_CAP), notNegative(AF_REL_ERR, 2, "rel_err and abs_err")}),
        };
    }();
    return T;
}

// the first check of the call's row that does not hold, as the refusal the call answers; or none.  `as`: an entry point that makes another's
// checks in the same order and has no row of its own (pt_reproject_frame_moved_bilinear: the bilinear call's) — its name, in place of the row's
// name and prefix
inline Refused checkImageArgs(ImageCall call, const ImageArgs& a, const char* as = nullptr) {
    const ImageCallRow& row = imageCallTable()[call];
    for (const ArgCheck& k : row.checks)
        if (!holds(k, a)) return Refused{PT_ERR_ARG, std::string(as ? as : (k.own ? row.name : row.prefix)) + ": " + refusalText(k)};
    return {};
}

}  // namespace ptp
