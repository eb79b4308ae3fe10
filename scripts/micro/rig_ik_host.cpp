// rig_ik_host.cpp — the host route of include/pt_rig_ik.h in C++ on ONE core: walk the hierarchy for the world matrices (ptp::rigLocal and ptp::rigCompose,
// csrc/hip/pt_rig_rule.hpp: the world matrices alone, no records), then solve every constraint (ptp::rigIk, csrc/hip/pt_rig_ik_rule.hpp) in place on the locals.  No HIP, no device.
// Two uses:
//   as a shared library, scripts/rig_ik_bench.py calls rig_ik_host() between the download of the mixed locals and their upload: the route a
//     caller has without the header
//       g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared -o rig_ik_host.so scripts/micro/rig_ik_host.cpp
//   as a program (-DRIG_IK_HOST_MAIN), the walk and the solve alone over 65536 joints as 4096 sixteen-joint characters with four chains each,
//     the best of 20 with a steady clock
//       g++ -O2 -std=c++17 -ffp-contract=off -DRIG_IK_HOST_MAIN -o rig_ik_host scripts/micro/rig_ik_host.cpp && ./rig_ik_host
#include "../../pathtracer-0_amd/csrc/hip/pt_rig_ik_rule.hpp"

#include <vector>

// locals: n joints, solved in place.  The walk makes the world matrices alone (steps 1 and 2 of include/pt_rig.h): no inverse bind, no N and no
// record, which the solve does not read and pt_rig_pose_geometry remakes on the device.  Returns the world matrices' last float so that the walk
// is used
extern "C" float rig_ik_host(const int32_t* parent, size_t n, const pt_rig_ik_constraint* cons, const pt_rig_ik_goal* goals, size_t nCons, float* locals) {
    static std::vector<float> world;
    world.resize(12 * n);
    float L[12];
    for (size_t j = 0; j < n; j++) {                                  // (parents come first)
        float* W = world.data() + 12 * j;
        ptp::rigLocal(locals + PT_RIG_LOCAL_FLOATS * j, L);
        if (parent[j] < 0) { for (int f = 0; f < 12; f++) W[f] = L[f]; }
        else ptp::rigCompose(world.data() + 12 * (size_t)parent[j], L, W);
    }
    ptp::rigIk(parent, cons, goals, nCons, world.data(), locals);
    return n ? world[12 * n - 1] : 0.0f;
}

#ifdef RIG_IK_HOST_MAIN
#include <chrono>
#include <cmath>
#include <cstdio>

int main() {
    const size_t chars = 4096, per = 16, n = chars * per;
    const int32_t one[per] = {-1, 0, 1, 2, 2, 4, 5, 2, 7, 8, 0, 10, 11, 0, 13, 14};      // scripts/rig_ik_bench.py's character
    const int32_t tips[4] = {6, 9, 12, 15};
    std::vector<int32_t> parent(n);
    std::vector<float> rest(12 * n), locals(12 * n);
    std::vector<pt_rig_ik_constraint> cons(4 * chars);
    std::vector<pt_rig_ik_goal> goals(4 * chars);
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f - 0.5f; };      // [-0.5, 0.5)
    for (size_t c = 0; c < chars; c++)
        for (size_t j = 0; j < per; j++) {
            parent[per * c + j] = one[j] < 0 ? -1 : (int32_t)(per * c) + one[j];
            float* l = rest.data() + 12 * (per * c + j);
            for (int f = 0; f < 3; f++) l[f] = 0.3f + 0.2f * rnd();
            l[4] = 0.1f * rnd(); l[5] = 0.1f * rnd(); l[6] = 0.1f * rnd(); l[7] = 1.0f;
            l[8] = l[9] = l[10] = 1.0f;
        }
    for (size_t k = 0; k < 4 * chars; k++) {
        cons[k] = pt_rig_ik_constraint{PT_RIG_IK_TWO_BONE, (int32_t)(per * (k / 4)) + tips[k % 4], PT_RIG_IK_POLE, 0, {0.0f, 0.0f, 0.0f}, 0.0f};
        goals[k] = pt_rig_ik_goal{{1.0f + rnd(), 1.0f + rnd(), 1.0f + rnd()}, 1.0f, {3.0f * rnd(), 4.0f, 3.0f * rnd()}, 0.0f};
    }
    if (ptp::checkRigIkAttach(true, cons.data(), cons.size() * sizeof(pt_rig_ik_constraint), parent.data(), (int)n).code) { std::printf("the table is refused\n"); return 1; }
    double best = 1e30, sum = 0.0;
    for (int k = 0; k < 20; k++) {
        locals = rest;
        const auto t0 = std::chrono::steady_clock::now();
        sum += rig_ik_host(parent.data(), n, cons.data(), goals.data(), cons.size(), locals.data());
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms < best) best = ms;
        sum += locals[12 * (n - 2) + 4];                              // the result is used
    }
    std::printf("host walk and solve: the world matrices + ptp::rigIk, %zu joints, %zu constraints: best of 20 %.2f ms on one core%s\n", n, cons.size(), best,
                std::isfinite(sum) ? "" : " [not finite]");
    return 0;
}
#endif
