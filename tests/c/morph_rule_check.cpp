// morph_rule_check.cpp — csrc/hip/pt_morph_rule.hpp on a CPU: reads one request per line and prints what the header answered.
//   A <live> <has morph> <target_start: 0|1> <entry_corner: 0|1> <entry_delta: 0|1> <n_targets> <start_bytes> <corner_bytes> <delta_bytes> <n_tris>
//     <n starts> <start> x n  <n corners> <corner> x n  <n delta floats> <delta word> x n  <moved: 0|1> x 3 n_tris
//                                                                                             -> <code> <MorphCheck> <text>     pt_morph_attach
//   W <live> <has morph> <weights: 0|1> <weight_bytes> <n_targets> <n weights> <weight word> x n  -> <code> <MorphCheck> <text>     pt_morph_weights
//   R <n_tris> <n_targets> <start> x (n_targets + 1) <corner> x E <delta word> x 6 E <rest word> x 40 n_tris <weight word> x n_targets
//                                  -> <n affected> <E> <corner> x n affected <row start> x (n affected + 1) <target> x E <delta word> x 6 E <pad> x E
//                                     and the 40 n_tris words of morphTriangles
// The arrays of A and W hold exactly the counts given, so that the sanitizer sees a read past them.  The floats travel as the hexadecimal words of
// their binary32 patterns, so that a NaN, a -0 and a denormal arrive as they were meant.
// Built by tests/test_morph_rule.py with g++, plain and under the address / undefined-behaviour sanitizers; no HIP, no device.
#include "../../pathtracer-0_amd/csrc/hip/pt_morph_rule.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <vector>

static float fromBits(const std::string& hex) {
    const uint32_t u = (uint32_t)std::stoul(hex, nullptr, 16);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static uint32_t toBits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s requests.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line, w;
    int64_t dummy64 = 0;
    int32_t dummy32 = 0;
    float fdummy = 0.0f;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream s(line);
        std::string kind;
        s >> kind;
        auto bad = [&]() { std::fprintf(stderr, "bad line: %.80s\n", line.c_str()); return 2; };
        auto floats = [&](std::vector<float>& v) {
            for (auto& x : v) { if (!(s >> w)) return false; x = fromBits(w); }
            return true;
        };
        if (kind == "A") {
            int live = 0, has = 0, pStart = 0, pCorner = 0, pDelta = 0, nTargets = 0, which = -1;
            size_t startBytes = 0, cornerBytes = 0, deltaBytes = 0, nTris = 0, n = 0;
            if (!(s >> live >> has >> pStart >> pCorner >> pDelta >> nTargets >> startBytes >> cornerBytes >> deltaBytes >> nTris)) return bad();
            if (!(s >> n)) return bad();
            std::vector<int64_t> starts(n);
            for (auto& v : starts) if (!(s >> v)) return bad();
            if (!(s >> n)) return bad();
            std::vector<int32_t> corners(n);
            for (auto& v : corners) if (!(s >> v)) return bad();
            if (!(s >> n)) return bad();
            std::vector<float> deltas(n);
            if (!floats(deltas)) return bad();
            std::vector<unsigned char> moved(3 * nTris);
            for (auto& v : moved) { int m = 0; if (!(s >> m)) return bad(); v = (unsigned char)m; }
            const ptp::Refused a = ptp::checkMorphAttach(live != 0, has != 0, nTargets, pStart ? (starts.empty() ? &dummy64 : starts.data()) : nullptr, startBytes,
                                                         pCorner ? (corners.empty() ? &dummy32 : corners.data()) : nullptr, cornerBytes,
                                                         pDelta ? (deltas.empty() ? &fdummy : deltas.data()) : nullptr, deltaBytes, nTris, moved.data(), &which);
            std::cout << a.code << ' ' << which << ' ' << a.msg << '\n';
        } else if (kind == "W") {
            int live = 0, has = 0, pW = 0, nTargets = 0, which = -1;
            size_t bytes = 0, n = 0;
            if (!(s >> live >> has >> pW >> bytes >> nTargets >> n)) return bad();
            std::vector<float> ws(n);
            if (!floats(ws)) return bad();
            const ptp::Refused a = ptp::checkMorphWeights(live != 0, has != 0, pW ? (ws.empty() ? &fdummy : ws.data()) : nullptr, bytes, nTargets, &which);
            std::cout << a.code << ' ' << which << ' ' << a.msg << '\n';
        } else if (kind == "R") {
            size_t nTris = 0;
            int nTargets = 0;
            if (!(s >> nTris >> nTargets)) return bad();
            std::vector<int64_t> starts((size_t)nTargets + 1);
            for (auto& v : starts) if (!(s >> v)) return bad();
            const size_t E = (size_t)starts.back();
            std::vector<int32_t> corners(E);
            for (auto& v : corners) if (!(s >> v)) return bad();
            std::vector<float> deltas(6 * E), rest(40 * nTris), ws((size_t)nTargets), out(40 * nTris);
            if (!floats(deltas) || !floats(rest) || !floats(ws)) return bad();
            std::vector<unsigned char> moved(3 * nTris, 1);
            int which = -1;
            if (ptp::checkMorphAttach(true, false, nTargets, starts.data(), starts.size() * 8, corners.data(), E * 4, deltas.data(), E * 24, nTris, moved.data(), &which).code ||
                ptp::checkMorphWeights(true, true, ws.data(), ws.size() * 4, nTargets, &which).code)
                return bad();                                            // the rule is stated for checked tables only
            ptp::MorphRows rows;
            ptp::morphRows(nTargets, starts.data(), corners.data(), deltas.data(), 3 * nTris, rows);
            ptp::morphTriangles(rest.data(), nTris, rows, ws.data(), out.data());
            std::string text = std::to_string(rows.corners.size()) + " " + std::to_string(rows.entries.size()) + " ";
            char word[16];
            for (int32_t v : rows.corners) text += std::to_string(v) + " ";
            for (int32_t v : rows.rowStart) text += std::to_string(v) + " ";
            for (const auto& e : rows.entries) text += std::to_string(e.target) + " ";
            for (const auto& e : rows.entries)
                for (float v : e.d) { std::snprintf(word, sizeof word, "%08x ", toBits(v)); text += word; }
            for (const auto& e : rows.entries) text += std::to_string(e.pad) + " ";
            for (float v : out) { std::snprintf(word, sizeof word, "%08x ", toBits(v)); text += word; }
            std::cout << text << '\n';
        } else return bad();
    }
    return 0;
}
