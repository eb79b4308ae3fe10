// despeckle_rule_check.cpp — csrc/hip/pt_despeckle_rule.hpp on a CPU: reads one call per line and prints what the check answered.
//   <entry point> <ctx: 0|1> <rule: 0|1> <radius> <sigmas bits> <min_taps> <own_z bits> <normal_tol bits> <min_lum bits>
// The floats travel as the hexadecimal words of their binary32 patterns, so that a NaN, a -0 and a denormal arrive as they were meant.  Answer:
//   <code> <DespeckleCheck> <text>
// Built by tests/test_despeckle_rule.py with g++, plain and under the address / undefined-behaviour sanitizers; no HIP, no device.
#include "../../pathtracer-0_amd/csrc/hip/pt_despeckle_rule.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

static float fromBits(const std::string& hex) {
    const uint32_t u = (uint32_t)std::stoul(hex, nullptr, 16);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s calls.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    int dummy = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream s(line);
        std::string who, sig, oz, nt, ml;
        int ctx = 0, rule = 0;
        pt_despeckle_rule r{};
        if (!(s >> who >> ctx >> rule >> r.radius >> sig >> r.min_taps >> oz >> nt >> ml)) { std::fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        r.sigmas = fromBits(sig); r.own_z = fromBits(oz); r.normal_tol = fromBits(nt); r.min_lum = fromBits(ml);
        int which = -1;
        const ptp::Refused a = ptp::checkDespeckleRule(who.c_str(), ctx ? &dummy : nullptr, rule ? &r : nullptr, &which);
        std::cout << a.code << ' ' << which << ' ' << a.msg << '\n';
    }
    return 0;
}
