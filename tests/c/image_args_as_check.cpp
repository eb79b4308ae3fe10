// image_args_as_check.cpp — the three-argument checkImageArgs of csrc/hip/pt_image_args.hpp (an entry point that makes another row's checks under its own
// name: pt_reproject_frame_moved_bilinear asks the bilinear row) held to the two-argument one on the CPU, over the bilinear row's fields at and
// around each bound and with each pointer absent.  tests/test_motion_bilinear_abi.py builds it with g++, plain and under the host sanitizers, and
// reads the lines it prints:
//   case WHAT rc=.. two=TEXT | three=TEXT
// Exit status 1 when a three-argument answer is not the two-argument one's code and text with the name replaced, or when a two-argument answer is
// not the one written down here.
#include "../../pathtracer-0_amd/csrc/hip/pt_image_args.hpp"

#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

namespace {

using namespace ptp;

const char* const ROW = "pt_reproject_frame_bilinear";
const char* const AS = "pt_reproject_frame_moved_bilinear";
int failures = 0;

ImageArgs good() {
    ImageArgs a;
    a.present = AP_CTX | AP_RULE;
    a.reproject(64.0f, 0.02f, 0.9f, 0, 0.0f);
    a.snap = 1.0f / 64.0f;
    return a;
}

// `tail`: the text the two-argument form has answered since the row was written, without its "NAME: "; "" = accepted
void expect(const char* what, const ImageArgs& a, const char* tail) {
    const Refused two = checkImageArgs(IC_REPROJECT_FRAME_BILINEAR, a), three = checkImageArgs(IC_REPROJECT_FRAME_BILINEAR, a, AS);
    const Refused again = checkImageArgs(IC_REPROJECT_FRAME_BILINEAR, a, nullptr);
    const std::string t(tail);
    const std::string wantTwo = t.empty() ? "" : std::string(ROW) + ": " + t, wantThree = t.empty() ? "" : std::string(AS) + ": " + t;
    const int wantCode = t.empty() ? 0 : PT_ERR_ARG;
    const bool ok = two.code == wantCode && three.code == wantCode && again.code == wantCode && two.msg == wantTwo && three.msg == wantThree && again.msg == wantTwo;
    std::printf("case %s rc=%d two=%s | three=%s%s\n", what, two.code, two.msg.c_str(), three.msg.c_str(), ok ? "" : "  MISMATCH");
    if (!ok) failures++;
}

template <class F>
void with(const char* what, F set, const char* tail) {
    ImageArgs a = good();
    set(a);
    expect(what, a, tail);
}

}  // namespace

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const char* const SNAP = "rule.snap must be in [0, 0.5)";
    const char* const FLOOR = "rule.albedo_floor must be 0 or finite and > 0";
    const char* const HIST = "max_history must be >= 1";
    const char* const DEPTH = "depth_tol must be > 0";
    const char* const NORMAL = "normal_tol must be in [-1, 1]";
    expect("good", good(), "");
    // each pointer absent, and both
    with("no_ctx", [](ImageArgs& a) { a.present = AP_RULE; }, "null argument");
    with("no_rule", [](ImageArgs& a) { a.present = AP_CTX; }, "null argument");
    with("no_pointer", [](ImageArgs& a) { a.present = 0; }, "null argument");
    with("other_pointers_only", [](ImageArgs& a) { a.present = AP_BUFFER | AP_THRU | AP_SEEDS | AP_MASK; }, "null argument");
    // snap in [0, 0.5)
    with("snap_0", [](ImageArgs& a) { a.snap = 0.0f; }, "");
    with("snap_minus_0", [](ImageArgs& a) { a.snap = -0.0f; }, "");
    with("snap_below_0", [](ImageArgs& a) { a.snap = std::nextafterf(0.0f, -1.0f); }, SNAP);
    with("snap_below_half", [](ImageArgs& a) { a.snap = std::nextafterf(0.5f, 0.0f); }, "");
    with("snap_half", [](ImageArgs& a) { a.snap = 0.5f; }, SNAP);
    with("snap_nan", [nan](ImageArgs& a) { a.snap = nan; }, SNAP);
    with("snap_inf", [inf](ImageArgs& a) { a.snap = inf; }, SNAP);
    with("snap_minus_inf", [inf](ImageArgs& a) { a.snap = -inf; }, SNAP);
    // albedo_floor 0 or finite and > 0
    with("floor_minus_0", [](ImageArgs& a) { a.albedo_floor = -0.0f; }, "");
    with("floor_denormal", [](ImageArgs& a) { a.albedo_floor = std::nextafterf(0.0f, 1.0f); }, "");
    with("floor_below_0", [](ImageArgs& a) { a.albedo_floor = std::nextafterf(0.0f, -1.0f); }, FLOOR);
    with("floor_max", [](ImageArgs& a) { a.albedo_floor = std::numeric_limits<float>::max(); }, "");
    with("floor_inf", [inf](ImageArgs& a) { a.albedo_floor = inf; }, FLOOR);
    with("floor_nan", [nan](ImageArgs& a) { a.albedo_floor = nan; }, FLOOR);
    // the four common ones
    with("history_1", [](ImageArgs& a) { a.max_history = 1.0f; }, "");
    with("history_below_1", [](ImageArgs& a) { a.max_history = std::nextafterf(1.0f, 0.0f); }, HIST);
    with("history_inf", [inf](ImageArgs& a) { a.max_history = inf; }, "");
    with("history_nan", [nan](ImageArgs& a) { a.max_history = nan; }, HIST);
    with("depth_0", [](ImageArgs& a) { a.depth_tol = 0.0f; }, DEPTH);
    with("depth_denormal", [](ImageArgs& a) { a.depth_tol = std::nextafterf(0.0f, 1.0f); }, "");
    with("depth_inf", [inf](ImageArgs& a) { a.depth_tol = inf; }, "");
    with("depth_nan", [nan](ImageArgs& a) { a.depth_tol = nan; }, DEPTH);
    with("normal_minus_1", [](ImageArgs& a) { a.normal_tol = -1.0f; }, "");
    with("normal_1", [](ImageArgs& a) { a.normal_tol = 1.0f; }, "");
    with("normal_above_1", [](ImageArgs& a) { a.normal_tol = std::nextafterf(1.0f, 2.0f); }, NORMAL);
    with("normal_below_minus_1", [](ImageArgs& a) { a.normal_tol = std::nextafterf(-1.0f, -2.0f); }, NORMAL);
    with("normal_nan", [nan](ImageArgs& a) { a.normal_tol = nan; }, NORMAL);
    with("flags_all_materials", [](ImageArgs& a) { a.flags = PT_REPROJECT_ALL_MATERIALS; }, "");
    with("flags_2", [](ImageArgs& a) { a.flags = 2; }, "unknown flags");
    with("flags_minus_1", [](ImageArgs& a) { a.flags = -1; }, "unknown flags");
    // the order of the checks: the first that does not hold answers
    with("order_pointer_first", [nan](ImageArgs& a) { a.present = AP_CTX; a.snap = nan; a.flags = 2; }, "null argument");
    with("order_snap_before_floor", [nan](ImageArgs& a) { a.snap = 0.5f; a.albedo_floor = nan; a.max_history = 0.0f; }, SNAP);
    with("order_floor_before_history", [nan](ImageArgs& a) { a.albedo_floor = nan; a.max_history = 0.0f; }, FLOOR);
    with("order_history_before_depth", [](ImageArgs& a) { a.max_history = 0.0f; a.depth_tol = 0.0f; a.normal_tol = 2.0f; a.flags = 2; }, HIST);
    with("order_normal_before_flags", [](ImageArgs& a) { a.normal_tol = 2.0f; a.flags = 2; }, NORMAL);
    // rows whose prefix or `own` mark differs from their name: the replacement covers both
    {
        ImageArgs a = ImageArgs::given(&a);
        a.reproject(0.5f, 0.02f, 0.9f, 0, 0.2f);
        const Refused two = checkImageArgs(IC_REPROJECT_FRAME_DEMOD, a), three = checkImageArgs(IC_REPROJECT_FRAME_DEMOD, a, "x");
        const bool ok = two.msg == "pt_reproject_frame: max_history must be >= 1" && three.msg == "x: max_history must be >= 1" && two.code == three.code;
        a.albedo_floor = 0.0f;
        const Refused own2 = checkImageArgs(IC_REPROJECT_FRAME_DEMOD, a), own3 = checkImageArgs(IC_REPROJECT_FRAME_DEMOD, a, "x");
        const bool ok2 = own2.msg == "pt_reproject_frame_demod: albedo_floor must be finite and > 0" && own3.msg == "x: albedo_floor must be finite and > 0";
        std::printf("case prefix_and_own rc=%d two=%s | three=%s%s\n", two.code, own2.msg.c_str(), own3.msg.c_str(), ok && ok2 ? "" : "  MISMATCH");
        if (!(ok && ok2)) failures++;
    }
    std::printf("%d mismatches\n", failures);
    return failures ? 1 : 0;
}
