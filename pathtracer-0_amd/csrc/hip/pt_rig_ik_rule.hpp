// pt_rig_ik_rule.hpp — the host-only part of include/pt_rig_ik.h: what its calls refuse in their arguments before their first HIP call (the first
// failing check as a code and one text each, in the header's order), the independence check on the parent array, the 16-byte row a constraint
// becomes on the device, the level window of a table, and ptp::rigIk, the CPU statement of the rule over a whole table (its steps per constraint
// are pt_rig_ik_steps.hpp's, which k_rig_ik shares).  Plain C++: no HIP runtime call and no context, so tests/c/rig_ik_rule_check.cpp runs all of
// it on a CPU.  Whether a rig is live is the registry's to say (pt_rig_host.hpp); it arrives here as an answer.  Compiled with -ffp-contract=off
// wherever it is compiled.
#pragma once
#include "../../../include/pt_rig_ik.h"
#include "pt_rig_ik_steps.hpp"
#include "pt_rig_rule.hpp"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace ptp {

// every check below, in the order the header lists them (the test requires each of them of its grid)
enum RigIkCheck { RK_OK, RK_RIG, RK_BYTES, RK_NULL, RK_KIND, RK_JOINT, RK_CHAIN, RK_FLAGS, RK_AXIS, RK_INDEPENDENT, RK_GOALS_NULL, RK_GOAL_BYTES, RK_WEIGHT,
                  RK_LOCALS, RK_LOCAL_BYTES, RK_OUT, RK_OUT_BYTES, RK_COUNT };

namespace rig_ik_detail {
inline Refused refuse(const char* who, int* which, RigIkCheck k, const std::string& text) {
    if (which) *which = k;
    return Refused{PT_ERR_ARG, std::string(who) + ": " + text};
}
}  // namespace rig_ik_detail

// the joints of a constraint that passed its own checks: (first's parent or -1, root, mid, tip), or (parent, joint, -1, -1) for AIM — the row the
// device reads, so that no lane walks the hierarchy
struct RigIkRow { int32_t parent, a, b, c; };
inline RigIkRow rigIkRow(const int32_t* parent, const pt_rig_ik_constraint& k) {
    if (k.kind == PT_RIG_IK_AIM) return RigIkRow{parent[k.joint], k.joint, -1, -1};
    const int32_t mid = parent[k.joint], root = parent[mid];
    return RigIkRow{parent[root], root, mid, k.joint};
}

// INDEPENDENCE: the index of the first constraint B that reads a joint another constraint writes, or -1.  The constraints passed their own checks
inline int rigIkDependent(const int32_t* parent, size_t nParts, const pt_rig_ik_constraint* cons, size_t nCons) {
    std::vector<int32_t> writer(nParts, -1);                          // the first constraint that writes the joint; -2: several do
    auto wrote = [&](int32_t j, int32_t by) { writer[(size_t)j] = writer[(size_t)j] == -1 ? by : -2; };
    for (size_t k = 0; k < nCons; k++) {
        const RigIkRow r = rigIkRow(parent, cons[k]);
        wrote(r.a, (int32_t)k);
        if (cons[k].kind == PT_RIG_IK_TWO_BONE) wrote(r.b, (int32_t)k);
    }
    auto foreign = [&](int32_t j, size_t by) { return writer[(size_t)j] != -1 && writer[(size_t)j] != (int32_t)by; };
    for (size_t k = 0; k < nCons; k++) {
        const RigIkRow r = rigIkRow(parent, cons[k]);
        if (foreign(r.a, k) || (r.b >= 0 && foreign(r.b, k)) || (r.c >= 0 && foreign(r.c, k))) return (int)k;
        for (int32_t j = r.parent; j >= 0; j = parent[j])
            if (foreign(j, k)) return (int)k;
    }
    return -1;
}

// pt_rig_ik_attach; live: the rig is neither null nor destroyed; parent and nParts: the rig's (read only when live)
inline Refused checkRigIkAttach(bool live, const pt_rig_ik_constraint* cons, size_t bytes, const int32_t* parent, int nParts, int* which = nullptr) {
    using rig_ik_detail::refuse;
    const char* who = "pt_rig_ik_attach";
    if (which) *which = RK_OK;
    if (!live) return refuse(who, which, RK_RIG, "null or destroyed rig");
    if (bytes % sizeof(pt_rig_ik_constraint)) return refuse(who, which, RK_BYTES, "bytes must be a multiple of 32");
    if (!cons && bytes > 0) return refuse(who, which, RK_NULL, "null constraints with bytes > 0");
    const size_t n = bytes / sizeof(pt_rig_ik_constraint);
    for (size_t k = 0; k < n; k++) {
        const pt_rig_ik_constraint& c = cons[k];
        const std::string at = "constraint " + std::to_string(k) + ": ";
        if (c.kind != PT_RIG_IK_TWO_BONE && c.kind != PT_RIG_IK_AIM) return refuse(who, which, RK_KIND, at + "unknown kind");
        if (c.joint < 0 || c.joint >= nParts) return refuse(who, which, RK_JOINT, at + "a joint outside [0, n_parts)");
        if (c.kind == PT_RIG_IK_TWO_BONE && (parent[c.joint] < 0 || parent[parent[c.joint]] < 0))
            return refuse(who, which, RK_CHAIN, at + "a tip without a parent and a grandparent");
        if (c.flags & ~PT_RIG_IK_POLE) return refuse(who, which, RK_FLAGS, at + "flags other than 0 or PT_RIG_IK_POLE");
        if (c.kind == PT_RIG_IK_AIM) {
            const double x = c.axis[0], y = c.axis[1], z = c.axis[2];
            const bool finite = std::isfinite(c.axis[0]) && std::isfinite(c.axis[1]) && std::isfinite(c.axis[2]);
            if (!finite || !(std::fabs(std::sqrt(x * x + y * y + z * z) - 1.0) <= 1e-3)) return refuse(who, which, RK_AXIS, at + "an axis that is not finite or not of length 1");
        }
    }
    const int dep = rigIkDependent(parent, (size_t)nParts, cons, n);
    if (dep >= 0) return refuse(who, which, RK_INDEPENDENT, "constraint " + std::to_string(dep) + " reads a joint that another constraint writes");
    return {};
}

// pt_rig_ik_goals; nCons: the table's constraints (read only when live)
inline Refused checkRigIkGoals(bool live, const pt_rig_ik_goal* goals, size_t bytes, size_t nCons, int* which = nullptr) {
    using rig_ik_detail::refuse;
    const char* who = "pt_rig_ik_goals";
    if (which) *which = RK_OK;
    if (!live) return refuse(who, which, RK_RIG, "null or destroyed rig");
    if (!goals && bytes > 0) return refuse(who, which, RK_GOALS_NULL, "null goals with bytes > 0");
    if (!goals) return {};                                            // (NULL, 0): off
    if (bytes != nCons * sizeof(pt_rig_ik_goal)) return refuse(who, which, RK_GOAL_BYTES, "bytes != 32 * the table's constraints");
    for (size_t k = 0; k < nCons; k++)
        if (!(std::isfinite(goals[k].weight) && goals[k].weight >= 0.0f && goals[k].weight <= 1.0f))
            return refuse(who, which, RK_WEIGHT, "goal " + std::to_string(k) + ": a weight must be finite and in [0, 1]");
    return {};
}

// pt_rig_ik_locals
inline Refused checkRigIkLocals(bool live, const float* locals, size_t localBytes, const float* out, size_t outBytes, int nParts, int* which = nullptr) {
    using rig_ik_detail::refuse;
    const char* who = "pt_rig_ik_locals";
    if (which) *which = RK_OK;
    if (!live) return refuse(who, which, RK_RIG, "null or destroyed rig");
    if (!locals && nParts > 0) return refuse(who, which, RK_LOCALS, "null locals with n_parts > 0");
    if (localBytes != (size_t)nParts * (PT_RIG_LOCAL_FLOATS * 4)) return refuse(who, which, RK_LOCAL_BYTES, "local_bytes != n_parts * 48");
    if (!out) return refuse(who, which, RK_OUT, "null locals_out");
    if (outBytes != (size_t)nParts * (PT_RIG_LOCAL_FLOATS * 4)) return refuse(who, which, RK_OUT_BYTES, "out_bytes != n_parts * 48");
    return {};
}

// THE LEVEL WINDOW of a table.  With level l holding the joints of depth l + 1 (ptp::RigPlan): the solve reads the world matrices of the first
// joints' parents, which the levels [0, before) make, and changes locals from level `from` on, so the levels [from, levels) run (again) after
// it.  before is the largest and from the smallest level of any first joint; the levels below `from` are made once, and those in [from, before)
// twice, the second time for good.  No constraints: nothing before, everything after
struct RigIkWindow { int before = 0, from = 0; };
inline RigIkWindow rigIkWindow(const int32_t* parent, size_t nParts, const pt_rig_ik_constraint* cons, size_t nCons) {
    RigIkWindow w;
    if (!nCons) return w;
    std::vector<int32_t> depth(nParts);
    rigDepths(parent, nParts, depth.data());
    int lo = 0, hi = 0;
    for (size_t k = 0; k < nCons; k++) {
        const int level = depth[(size_t)rigIkRow(parent, cons[k]).a] - 1;
        if (k == 0 || level < lo) lo = level;
        if (k == 0 || level > hi) hi = level;
    }
    w.before = hi; w.from = lo;
    return w;
}

// THE RULE over a table: world holds the first pass's world matrices (12 floats per joint: ptp::rigRecords' world of these locals), locals are
// changed in place.  The constraints are independent, so their order does not matter
inline void rigIk(const int32_t* parent, const pt_rig_ik_constraint* cons, const pt_rig_ik_goal* goals, size_t nCons, const float* world, float* locals) {
    constexpr size_t F = PT_RIG_LOCAL_FLOATS;
    for (size_t k = 0; k < nCons; k++) {
        const RigIkRow r = rigIkRow(parent, cons[k]);
        const bool hasP = r.parent >= 0;
        const float* P = hasP ? world + 12 * (size_t)r.parent : world;
        const pt_rig_ik_goal& g = goals[k];
        if (cons[k].kind == PT_RIG_IK_AIM) {
            float q[4];
            if (ptik::aim(P, hasP, locals + F * (size_t)r.a, cons[k].axis, g.target, g.weight, q))
                for (int f = 0; f < 4; f++) locals[F * (size_t)r.a + 4 + (size_t)f] = q[f];
            continue;
        }
        float q0[4], q1[4];
        if (ptik::twoBone(P, hasP, locals + F * (size_t)r.a, locals + F * (size_t)r.b, locals + F * (size_t)r.c, g.target, g.pole, (cons[k].flags & PT_RIG_IK_POLE) != 0, g.weight, q0, q1))
            for (int f = 0; f < 4; f++) { locals[F * (size_t)r.a + 4 + (size_t)f] = q0[f]; locals[F * (size_t)r.b + 4 + (size_t)f] = q1[f]; }
    }
}

}  // namespace ptp
