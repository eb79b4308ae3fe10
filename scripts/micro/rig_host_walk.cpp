// rig_host_walk.cpp — what the walk of include/pt_rig.h costs on ONE host core in C++: ptp::rigRecords (csrc/hip/pt_rig_rule.hpp, the CPU
// statement of steps 1-4) over 65536 joints, flat and as 4096 chains of depth 16, the best of 20 with a steady clock.  No HIP, no device: the
// figure scripts/rig_bench.py puts beside the numpy model's and beside pt_rig_pose_geometry's call.
//   g++ -O2 -std=c++17 -ffp-contract=off -o rig_host_walk scripts/micro/rig_host_walk.cpp && ./rig_host_walk
#include "../../pathtracer-0_amd/csrc/hip/pt_rig_rule.hpp"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>

int main() {
    const size_t n = 65536, depth = 16;
    std::vector<float> locals(12 * n), world(12 * n), records(24 * n);
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f - 0.5f; };      // [-0.5, 0.5)
    for (size_t j = 0; j < n; j++) {
        float* l = locals.data() + 12 * j;
        for (int f = 0; f < 3; f++) l[f] = 0.01f * rnd();
        l[4] = 0.01f * rnd(); l[5] = 0.01f * rnd(); l[6] = 0.01f * rnd(); l[7] = 1.0f;
        l[8] = l[9] = l[10] = 1.0f;
    }
    for (int chains = 0; chains < 2; chains++) {
        std::vector<int32_t> parent(n);
        for (size_t j = 0; j < n; j++) parent[j] = chains && j % depth ? (int32_t)j - 1 : -1;
        double best = 1e30, sum = 0.0;
        for (int k = 0; k < 20; k++) {
            const auto t0 = std::chrono::steady_clock::now();
            ptp::rigRecords(parent.data(), n, nullptr, locals.data(), world.data(), records.data());
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (ms < best) best = ms;
            sum += records[24 * (n - 1) + 12];                       // the result is used
        }
        std::printf("host walk: ptp::rigRecords, %zu joints, %s: best of 20 %.2f ms on one core (%.0f ns per joint)%s\n", n, chains ? "4096 chains of depth 16" : "flat", best,
                    best * 1e6 / (double)n, std::isfinite(sum) ? "" : " [not finite]");
    }
    return 0;
}
