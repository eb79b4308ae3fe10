// pt_refit_plan.hpp — the host-only planning of a BVH refit (include/pt_refit.h): every refusal of pt_refit_create with its text, the parent of
// every node, its height (a leaf is 0, an inner node 1 + the larger of its children's) and the reachable nodes grouped by height, which is the order
// the kernels of pt_refit.hip run them in.  Plain C++: no HIP runtime call.  pt_refit_create (pt_refit.hip) uploads the result;
// tests/c/refit_plan_check.cpp runs it on the CPU.
#pragma once
#include "../../../include/pt_refit.h"

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace ptr {

constexpr int64_t MAX_NODES = 1ll << 27, MAX_TRIS = 1ll << 30, MAX_LEAF_IDX = 1ll << 30;
constexpr int TAIL_BLOCK = 256;                      // lanes of a refit block; the upper heights run in one block of it once they fit (tailFrom)

struct RefitInput {
    const float* data = nullptr; size_t dataBytes = 0;        // binding 10
    const int32_t* tree = nullptr; size_t treeBytes = 0;      // binding 11
    const int32_t* leaf = nullptr; size_t leafBytes = 0;      // binding 12
    const int32_t* roots = nullptr; size_t rootsBytes = 0;    // binding 13
    int64_t nTris = 0;
};

struct RefitSchedule {
    int nNodes = 0, nRows = 0, nLeafIdx = 0, nRoots = 0;      // rows of binding 11 / of binding 10
    std::vector<int32_t> parent;                     // per node: its parent, -1 for a root and for a node no root reaches
    std::vector<int32_t> height;                     // per node: -1 when no root reaches it
    std::vector<int32_t> order;                      // the reachable nodes, by height ascending and by id within a height
    std::vector<int32_t> levelStart;                 // height h is order[levelStart[h] .. levelStart[h + 1]); maxHeight + 2 entries
    std::vector<int32_t> roots;                      // binding 13's roots in its order
    int maxHeight = -1;                              // -1: no reachable node
    int nLeaves() const { return levelStart.size() > 1 ? levelStart[1] : 0; }
    // the first height from which every remaining node fits one block: heights [1, tailFrom) get a launch each, [tailFrom, maxHeight] one launch
    int tailFrom() const {
        int h = maxHeight + 1;
        while (h > 1 && (int)order.size() - levelStart[h - 1] <= TAIL_BLOCK) h--;
        return h;
    }
};

// What a plan was made from, as 64 bits: bindings 11, 12 and 13 whole, floats 6 and 7 (the leaf ranges) of every row of binding 10, and the lengths
// of all four.  pt_refit_create keeps it; pt_move_geometry (include/pt_move.h) compares it with the same digest of a context's host copies.  Four
// multiplicative lanes over the 32-bit words, so that the multiplies of neighbouring words overlap; the values' bit patterns, never their order.
struct TopologyDigest {
    uint64_t h[4] = {0xcbf29ce484222325ull, 0x9e3779b97f4a7c15ull, 0xc2b2ae3d27d4eb4full, 0x165667b19e3779f9ull};
    size_t n = 0;
    void word(uint32_t w) { uint64_t& x = h[n++ & 3]; x = (x ^ w) * 0x100000001b3ull; }
    void words(const void* p, size_t count) {
        const unsigned char* q = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < count; i++) { uint32_t w; std::memcpy(&w, q + 4 * i, 4); word(w); }
    }
    void length(size_t v) { n = 0; word((uint32_t)v); word((uint32_t)((uint64_t)v >> 32)); }
    uint64_t value() const {
        uint64_t r = 0;
        for (int k = 0; k < 4; k++) { r = (r ^ h[k]) * 0x100000001b3ull; r ^= r >> 29; }
        return r;
    }
};
inline uint64_t topologyDigest(const int32_t* tree, size_t nTree, const int32_t* leaf, size_t nLeaf, const int32_t* roots, size_t nRoots, const float* data,
                               size_t nData) {
    TopologyDigest d;
    d.length(nTree); d.words(tree, nTree);
    d.length(nLeaf); d.words(leaf, nLeaf);
    d.length(nRoots); d.words(roots, nRoots);
    d.length(nData);
    for (size_t row = 0; row + 1 <= nData / 8; row++) d.words(data + 8 * row + 6, 2);
    return d.value();
}

inline int refitFail(std::string& err, int code, const char* msg) { err = std::string("pt_refit_create: ") + msg; return code; }

// 0, or PT_ERR_ARG / PT_ERR_SCENE with err set
inline int planRefit(const RefitInput& in, RefitSchedule& s, std::string& err) {
    if (!in.data || !in.tree || !in.leaf || !in.roots) return refitFail(err, PT_ERR_ARG, "null buffer");
    if (in.dataBytes % 32) return refitFail(err, PT_ERR_ARG, "data_bytes is not a multiple of 32 (8 floats per node)");
    if (in.treeBytes % 12) return refitFail(err, PT_ERR_ARG, "tree_bytes is not a multiple of 12 (3 ints per node)");
    if (in.leafBytes % 4) return refitFail(err, PT_ERR_ARG, "leaf_bytes is not a multiple of 4");
    if (in.rootsBytes % 4 || in.rootsBytes < 4) return refitFail(err, PT_ERR_ARG, "roots_bytes must be a multiple of 4 and hold the count");
    if (in.nTris < 0) return refitFail(err, PT_ERR_ARG, "n_tris is negative");
    if ((int64_t)(in.treeBytes / 12) > MAX_NODES || (int64_t)(in.dataBytes / 32) > MAX_NODES || in.nTris > MAX_TRIS || (int64_t)(in.leafBytes / 4) > MAX_LEAF_IDX)
        return refitFail(err, PT_ERR_ARG, "more than 2^27 nodes, 2^30 triangles or 2^30 leaf entries");
    const int n = (int)(in.treeBytes / 12), nLeafIdx = (int)(in.leafBytes / 4);
    s = RefitSchedule{};
    s.nNodes = n; s.nRows = (int)(in.dataBytes / 32); s.nLeafIdx = nLeafIdx;
    if (s.nRows < n) return refitFail(err, PT_ERR_SCENE, "BVHdata (binding 10) shorter than 8 floats per BVHtree node");
    // every row, reachable or not: ids, and children that lie behind their parent
    for (int i = 0; i < n; i++) {
        const int32_t* t = in.tree + 3 * (size_t)i;
        if (t[0] != i) return refitFail(err, PT_ERR_SCENE, "BVHtree row whose id is not its index");
        if (t[1] == -1 && t[2] == -1) continue;
        if (t[1] == -1 || t[2] == -1) return refitFail(err, PT_ERR_SCENE, "BVHtree node with one child without the other");
        for (int c = 1; c <= 2; c++)
            if (t[c] <= i || t[c] >= n) return refitFail(err, PT_ERR_SCENE, "BVHtree child outside (id, n_nodes)");
    }
    const int32_t count = in.roots[0];
    if (count < 0 || (size_t)count + 1 > in.rootsBytes / 4) return refitFail(err, PT_ERR_SCENE, "objIndices[0] exceeds the buffer");
    s.nRoots = count;
    s.parent.assign(n, -1); s.height.assign(n, -1);
    std::vector<char> reached(n, 0);
    for (int r = 0; r < count; r++) {
        const int32_t root = in.roots[1 + r];
        if (root < 0 || root >= n) return refitFail(err, PT_ERR_SCENE, "objIndices root out of range");
        if (reached[root]) return refitFail(err, PT_ERR_SCENE, "BVH node with two parents or reached from two roots");
        reached[root] = 1; s.roots.push_back(root);
    }
    // children lie behind their parents, so one pass in id order reaches everything a root reaches
    for (int i = 0; i < n; i++) {
        if (!reached[i]) continue;
        const int32_t* t = in.tree + 3 * (size_t)i;
        if (t[1] == -1) continue;
        for (int c = 1; c <= 2; c++) {
            if (reached[t[c]]) return refitFail(err, PT_ERR_SCENE, "BVH node with two parents or reached from two roots");
            reached[t[c]] = 1; s.parent[t[c]] = i;
        }
    }
    // ... and one pass against it gives the heights; the leaves' ranges on the way
    for (int i = n - 1; i >= 0; i--) {
        if (!reached[i]) continue;
        const int32_t* t = in.tree + 3 * (size_t)i;
        if (t[1] != -1) { s.height[i] = 1 + (s.height[t[1]] > s.height[t[2]] ? s.height[t[1]] : s.height[t[2]]); continue; }
        s.height[i] = 0;
        const float fs = in.data[8 * (size_t)i + 6], fe = in.data[8 * (size_t)i + 7];
        if (!(fs == std::floor(fs)) || !(fe == std::floor(fe)) || std::isinf(fs) || std::isinf(fe))
            return refitFail(err, PT_ERR_SCENE, "leaf range (floats 6 and 7 of BVHdata) is not integral");
        if (!(0.0f <= fs && fs <= fe && fe <= (float)nLeafIdx) || (int64_t)fe > nLeafIdx)
            return refitFail(err, PT_ERR_SCENE, "leaf range outside 0 <= start <= end <= leaf count");
        for (int k = (int)fs; k < (int)fe; k++)
            if (in.leaf[k] < 0 || in.leaf[k] >= in.nTris) return refitFail(err, PT_ERR_SCENE, "leafTriIndices entry outside [0, n_tris)");
    }
    for (int i = 0; i < n; i++) if (s.height[i] > s.maxHeight) s.maxHeight = s.height[i];
    // counting sort by height
    s.levelStart.assign((size_t)s.maxHeight + 2, 0);
    for (int i = 0; i < n; i++) if (s.height[i] >= 0) s.levelStart[(size_t)s.height[i] + 1]++;
    for (size_t h = 1; h < s.levelStart.size(); h++) s.levelStart[h] += s.levelStart[h - 1];
    s.order.assign((size_t)s.levelStart.back(), -1);
    std::vector<int32_t> fill(s.levelStart.begin(), s.levelStart.end() - 1);
    for (int i = 0; i < n; i++) if (s.height[i] >= 0) s.order[(size_t)fill[s.height[i]]++] = i;
    return 0;
}

}  // namespace ptr
