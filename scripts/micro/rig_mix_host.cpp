// rig_mix_host.cpp — what the mix of include/pt_rig_mix.h costs on ONE host core in C++: ptp::rigMix (csrc/hip/pt_rig_mix_rule.hpp, the CPU
// statement of steps 2-7) over 65536 joints with 2 and with 8 layers, the best of 20 with a steady clock.  No HIP, no device: the figure
// scripts/rig_mix_bench.py puts beside the numpy model's and beside pt_rig_mix_pose_geometry's call.  The layers are that script's: the base
// between two keys, then override and additive layers in turn, every one masked and between two keys.
//   g++ -O2 -std=c++17 -ffp-contract=off -o rig_mix_host scripts/micro/rig_mix_host.cpp && ./rig_mix_host
#include "../../pathtracer-0_amd/csrc/hip/pt_rig_mix_rule.hpp"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>

int main() {
    const size_t n = 65536;
    const int nKeys = 3;
    std::vector<float> keys[2], mask(n), out(12 * n);
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f - 0.5f; };      // [-0.5, 0.5)
    for (auto& clip : keys) {
        clip.resize(12 * n * nKeys);
        for (size_t j = 0; j < n * nKeys; j++) {
            float* l = clip.data() + 12 * j;
            for (int f = 0; f < 3; f++) l[f] = 0.01f * rnd();
            l[4] = 0.01f * rnd(); l[5] = 0.01f * rnd(); l[6] = 0.01f * rnd(); l[7] = 1.0f;
            l[8] = l[9] = l[10] = 1.0f;
        }
    }
    for (size_t j = 0; j < n; j++) mask[j] = (float)(j % 16) / 15.0f;
    for (int nLayers : {2, 8}) {
        std::vector<ptp::RigMixLayer> table((size_t)nLayers);
        for (int l = 0; l < nLayers; l++) {
            ptp::RigMixLayer& y = table[(size_t)l];
            const float* clip = keys[l % 2].data();
            y.a = clip + 12 * n * (size_t)(l % 2); y.b = y.a + 12 * n; y.r = clip;
            y.mask = l ? mask.data() : nullptr;
            y.u = 0.25f + 0.0625f * (float)l; y.weight = l ? 0.75f : 1.0f; y.mode = l % 2 ? PT_RIG_MIX_OVERRIDE : (l ? PT_RIG_MIX_ADDITIVE : PT_RIG_MIX_OVERRIDE);
        }
        double best = 1e30, sum = 0.0;
        for (int k = 0; k < 20; k++) {
            const auto t0 = std::chrono::steady_clock::now();
            ptp::rigMix(table.data(), nLayers, n, out.data());
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (ms < best) best = ms;
            sum += out[12 * (n - 1) + 4];                            // the result is used
        }
        std::printf("host mix: ptp::rigMix, %zu joints, %d layers: best of 20 %.2f ms on one core (%.0f ns per joint)%s\n", n, nLayers, best, best * 1e6 / (double)n,
                    std::isfinite(sum) ? "" : " [not finite]");
    }
    return 0;
}
