// pt_scene_layout.hpp — the host-only half of the scene build: validates the reference's buffers and lays out every device-private record array
// (pt_scene_records.hpp, pt_device.hpp) and the modes that depend on the scene.  No HIP runtime call and no context: buildScene (pt_context.hpp) uploads
// the result; tests/c/scene_layout_check.cpp runs it on the CPU.
#pragma once
#include "../../../include/pt_api.h"
#include "pt_scene_records.hpp"
#include "pt_launch_plan.hpp"

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace ptl {
using namespace ptd;

using LayoutOptions = ptp::Options;          // the layout reads the members whose rows of the option table say they rebuild the scene, and asmNodes80Limit
constexpr int EXTEND_BLOCK = 256;            // lanes of a k_extend block: one traversal stack each beside the LDS tile (BLOCK of pt_kernels.hpp)

// raw SSBO contents (host copies, glBufferData semantics)
struct SceneBuffers {
    std::vector<float> origin, rotation, mouse, tris, params, imp, ellip, bvhdata, mtl;
    std::vector<int32_t> bvhtree, leaftris, objidx;
    std::vector<uint8_t> sky; int skyW = 0, skyH = 0;
    struct HostTex { std::vector<uint8_t> rgba; int w = 0, h = 0; };
    std::vector<HostTex> textures;          // bindless table beyond the sky (index 0 mirrors `sky`)
};

struct SceneLayout {
    std::vector<float4> nodes, tris, shade;          // 64-B inner-node records, leaf-ordered triangle records, shading records by triangle id
    std::vector<float> nodes80;                      // node records of the hand-written kernel, asmNodeStride bytes each
    std::vector<int> triObj;
    std::vector<ObjRoot> roots;                      // numObj (at least 8) root records, then the 64 group boxes when numObj > 8
    std::vector<EllipRec> ellip; std::vector<MatRec> mats;
    std::vector<unsigned char> matVD;                // one flag byte per material: 1 = view-dependent (include/pt_reproject.h)
    std::vector<float> niDict;                       // the refraction-index dictionary, at least 8 entries
    std::vector<uint8_t> texels;                     // every texture beyond the sky, one block
    std::vector<size_t> texOff; std::vector<int> texW, texH;      // per entry of the texture table: first texel in the block, size (entry 0: the sky, not in the block)
    int nInner = 0, nTriRecs = 0, nTris = 0, numObj = 0, numEllip = 0, numMat = 0;
    bool trans = false, anySubsurface = false, anyMaps = false, ellipMaps = false, ambiguousTriObj = false;
    int niBits = 0; float ni8[8] = {};
    int stackDepth = 1, asmNodeStride = 80, asmGroupShift = 0, ldsNodes = 0, ldsTris = 0, stackMode = 2, pLdsNodes = 0, pLdsTris = 0;
    bool asmEligible = false; std::string asmWhyNot;

    // what the launch planner reads of it (pt_launch_plan.hpp)
    ptp::PlanScene planScene() const {
        ptp::PlanScene s;
        s.nNodes = nInner; s.nTriRecs = nTriRecs; s.numObj = numObj; s.stackDepth = stackDepth; s.stackMode = stackMode; s.asmNodeStride = asmNodeStride;
        s.ellipMaps = ellipMaps; s.asmEligible = asmEligible; s.ldsNodes = ldsNodes; s.ldsTris = ldsTris;
        return s;
    }
};

// (int)f of caller data with a defined result for every f: what the x86 conversion returns, INT_MIN for a NaN and for values outside int's range
inline int toInt(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT_MIN; }
inline float4 f4(float a, float b, float c, float d) { return make_float4(a, b, c, d); }
inline float asf(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

// ---- the per-record expressions that depend on the coordinates of binding 3 and the boxes of binding 10: the layout below and the in-place move
// (pt_scene_move.hpp, whose kernels in pt_move.hip evaluate the same binary32 expressions) both call them
// floats 0-8 of a triangle record (v1, e1, e2) from the 40 floats T of a triangle: r[0], r[1] and the first float of r[2]
inline void triRecordGeometry(const float* T, float4* r) {
    float e1x = T[4] - T[0], e1y = T[5] - T[1], e1z = T[6] - T[2], e2x = T[8] - T[0], e2y = T[9] - T[1], e2z = T[10] - T[2];
    r[0] = f4(T[0], T[1], T[2], e1x); r[1] = f4(e1y, e1z, e2x, e2y); r[2].x = e2z;
}
inline void shadeRecord(const float* T, float4* r) {
    r[0] = f4(T[12], T[13], T[14], T[16]); r[1] = f4(T[17], T[18], T[24], T[25]);
    r[2] = f4(T[28], T[29], T[32], asf((uint32_t)toInt(T[36]))); r[3] = f4(T[33], 0, 0, 0);
}
// the three box float4 of a 64-byte inner record from its children's rows A (left) and B (right) of binding 10
inline void nodeRecordBoxes(const float* A, const float* B, float4* r) {
    r[0] = f4(A[0], B[0], A[1], B[1]); r[1] = f4(A[2], B[2], A[3], B[3]); r[2] = f4(A[4], B[4], A[5], B[5]);
}
// the box floats of a record of the hand-written kernel (o: its first float, stride 80 or 64 bytes); false: a box with min > max or a NaN
inline bool node80RecordBoxes(const float* A, const float* B, float* o, int asmStride) {
    bool ordered = true;
    for (int ax = 0; ax < 3; ax++) {
        float* g = asmStride == 80 ? o + 2 + 6 * ax : o + 4 + 4 * ax;
        g[0] = A[ax]; g[1] = B[ax]; g[2] = A[3 + ax]; g[3] = B[3 + ax];
        if (asmStride == 80) { g[4] = A[ax]; g[5] = B[ax]; }
        if (!(A[ax] <= A[3 + ax]) || !(B[ax] <= B[3 + ax])) ordered = false;      // min > max or a NaN: only the min/max form of rayBox is right
    }
    return ordered;
}
inline void rootRecordBox(const float* A, ObjRoot& r) { for (int k = 0; k < 3; k++) { r.bmin[k] = A[k]; r.bmax[k] = A[3 + k]; } }
inline int cullGroupShift(int numObj) {
    int sft = 0;
    if (numObj > 8) while (((numObj + (1 << sft) - 1) >> sft) > 64) sft++;
    return sft;
}
// The 64 group boxes of more than 8 BVHs (rootsAndCullGroups below says what they promise).  root(o): the root node's row of binding 10; rootIsLeaf(o);
// child(o, side): the row of an inner root's child
template <class Root, class IsLeaf, class Child>
inline void cullGroups(int numObj, bool noRootCull, Root root, IsLeaf rootIsLeaf, Child child, std::vector<ObjRoot>& groups) {
    const int sft = cullGroupShift(numObj);
    const int nGroups = (numObj + (1 << sft) - 1) >> sft;
    const float inf = std::numeric_limits<float>::infinity();
    groups.assign(64, ObjRoot{});
    for (int g = 0; g < 64; g++) { for (int k = 0; k < 3; k++) { groups[g].bmin[k] = inf; groups[g].bmax[k] = -inf; } groups[g].ref = 0; groups[g].pad = 0; }
    for (int o = 0; o < numObj; o++) {
        const float* A = root(o);
        bool cullable = !rootIsLeaf(o) && !noRootCull;
        for (int k = 0; k < 3 && cullable; k++) {
            if (!(A[k] <= A[3 + k])) cullable = false;                                      // ordered, no NaN
            for (int side = 0; side < 2 && cullable; side++) {
                const float* Ch = child(o, side);
                // BOTH planes of the child inside the root's range: rayBox takes min / max of the two plane distances (:412-413), so an inverted child
                // (min > max) whose `max` lies below the root's min would stick out of the root although its `min` and `max` each pass a one-sided test (NaN: not)
                if (!(Ch[k] >= A[k] && Ch[k] <= A[3 + k] && Ch[3 + k] >= A[k] && Ch[3 + k] <= A[3 + k])) cullable = false;
            }
        }
        ObjRoot& G = groups[o >> sft];
        if (!cullable) G.pad = 1;
        for (int k = 0; k < 3; k++) { G.bmin[k] = std::min(G.bmin[k], A[k]); G.bmax[k] = std::max(G.bmax[k], A[3 + k]); }
    }
    for (int g = 0; g < nGroups; g++) if (groups[g].pad) { for (int k = 0; k < 3; k++) { groups[g].bmin[k] = -inf; groups[g].bmax[k] = inf; } }
}
// record i of the N ellipsoids of binding 7 (frag.glsl:606-611 layout); the material index is the caller's to check
inline void ellipRecord(const float* E, size_t N, size_t i, EllipRec& r) {
    std::memset(&r, 0, sizeof(r));
    for (int k = 0; k < 3; k++) { r.c[k] = E[1 + 3 * i + k]; r.st[k] = E[1 + N * 3 + 3 * i + k]; r.rot[k] = E[1 + N * 6 + 3 * i + k]; }
    r.r = E[1 + N * 9 + i]; r.mat = toInt(E[1 + N * 10 + i]);
}

// One run of layoutScene: the buffers, the result, and what the steps hand each other.  Each step returns 0 or fails with PT_ERR_SCENE and its text.
struct LayoutRun {
    const SceneBuffers& b; const LayoutOptions& opt; SceneLayout& L; std::string& err;
    size_t nTris = 0, nNodes = 0;
    int nMat = 0, numObj = 0, maxInnerDepth = -1;
    std::vector<int> newIdx, depth, objOf, leafRef;
    std::vector<int> order;                                     // inner nodes in multi-root BFS order
    std::vector<char> seen;
    bool boxesOrdered = true, anyEmpty = false;

    LayoutRun(const SceneBuffers& b_, const LayoutOptions& opt_, SceneLayout& L_, std::string& err_) : b(b_), opt(opt_), L(L_), err(err_) {}
    int fail(const char* msg) { err = msg; return PT_ERR_SCENE; }
    int childOf(int n, int side) const { return b.bvhtree[3 * (size_t)n + 1 + side]; }
    bool isLeaf(int n) const { return (childOf(n, 0) | childOf(n, 1)) == -1; }   // bitwise OR, frag.glsl:478
    int refOf(int n) const { return isLeaf(n) ? leafRef[n] : newIdx[n]; }
    const float* boxOf(int n) const { return b.bvhdata.data() + 8 * (size_t)n; }

    int presence() {
        nTris = b.tris.size() / 40; nNodes = b.bvhtree.size() / 3;
        if (b.params.size() < 12) return fail("Parameters buffer (binding 4) must hold 12 floats");
        if (b.origin.size() < 3 || b.rotation.size() < 3) return fail("ORIGIN/ROTATION (bindings 0,1) not set");
        if (b.mouse.size() < 3) return fail("MOUSE_POS (binding 2) not set");
        if (b.mtl.empty()) return fail("mtlData (binding 14) not set");
        if (b.objidx.empty()) return fail("objIndices (binding 13) not set");
        // Implicit surfaces: the reference loops over them (frag.glsl:578-605) and rayImplicit returns 1e30 before anything else (:385-386), so `t < closest_t` never passes —
        // they are never hit and leave no trace in the image.  The buffer is accepted as the reference's scene code sends it (dispatch.java:429-456) and otherwise unread.
        if (b.imp.empty() || !(b.imp[0] >= 0.0f)) return fail("ImpData (binding 5) not set: [count, fn x n, shift x 3n, scale x 3n, rot x 3n, mat x n]; send [0] for none");
        if (b.ellip.empty()) return fail("EllipData (binding 7) not set");
        if (b.sky.empty()) return fail("texture 0 (sky) not set");
        if (b.bvhdata.size() < 8 * nNodes) return fail("BVHdata shorter than 8 floats per BVHtree node");
        return 0;
    }

    int materials() {
        int me = toInt(b.mtl[0]);
        if (me < 48) return fail("mtlData[0] (floats per material) must be >= 48");
        nMat = (int)((b.mtl.size() - 1) / me);
        std::vector<MatRec>& mats = L.mats;
        mats.assign(std::max(nMat, 1), MatRec{});
        for (int m = 0; m < nMat; m++) {
            const float* F = b.mtl.data() + (size_t)me * m;      // F[k] == mtlData[me*m + k]
            MatRec& r = mats[m];
            // map_* slots of the 48-float record (dispatch.java:295-315): Ka 22, Kd 23, Ks 24, Pm 32, Pr 33, Pc 35, bump/norm 37, Tr 39, Ke 41
            // (map_Ps 34, map_Pcr 36, map_d 38, map_Ns 40 only change fields the render path never reads)
            r.map_Ka = toInt(F[22]); r.map_Kd = toInt(F[23]); r.map_Ks = toInt(F[24]); r.map_Pm = toInt(F[32]); r.map_Pr = toInt(F[33]); r.map_Pc = toInt(F[35]);
            r.map_norm = toInt(F[37]); r.map_Tr = toInt(F[39]); r.map_Ke = toInt(F[41]);
            r.hasMaps = 0;
            for (int idx : {r.map_Ka, r.map_Kd, r.map_Ks, r.map_Ke, r.map_Tr, r.map_Pm, r.map_Pr, r.map_Pc, r.map_norm}) {
                if (idx <= -1) continue;
                r.hasMaps = 1;
                if ((size_t)idx >= b.textures.size() || b.textures[idx].rgba.empty())
                    return fail("a material names a texture index that was never uploaded with pt_set_texture");
            }
            for (int k = 0; k < 3; k++) { r.Kd[k] = F[4 + k]; r.Ks[k] = F[7 + k]; r.Tf[k] = F[13 + k]; r.Ke[k] = F[17 + k]; }
            r.Tr = F[12]; r.Ni = F[16]; r.Density = F[20]; r.illum = toInt(F[21]); r.Pm = F[25]; r.Pr = F[26]; r.Pc = F[28]; r.Pcr = F[29]; r.subsurface = F[42];
            for (int k = 0; k < 3; k++) { r.Ka[k] = F[1 + k]; r.ssColor[k] = F[43 + k]; r.ssRadius[k] = F[46 + k]; }
            if (r.Tr > 0.0f || r.Tf[0] > 0.0f || r.illum == 5 || r.illum == 7 || r.map_Tr > -1) L.trans = true;   // (a Tr map can switch transmission on)
            if (r.subsurface > 0.0f) L.anySubsurface = true;
            if (r.hasMaps) L.anyMaps = true;
        }
        // the refraction-index dictionary (pt_device.hpp, DevScene::ni8): 0.0f, 1.0029f, then every distinct Ni bit pattern among the materials
        std::vector<float>& niDict = L.niDict;
        niDict = {0.0f, 1.0029f};
        for (int m = 0; m < nMat; m++) {
            uint32_t bits; std::memcpy(&bits, &mats[m].Ni, 4);
            int code = -1;
            for (size_t k = 0; k < niDict.size(); k++) { uint32_t kb; std::memcpy(&kb, &niDict[k], 4); if (kb == bits) { code = (int)k; break; } }
            if (code < 0) { code = (int)niDict.size(); niDict.push_back(mats[m].Ni); }
            mats[m].niCode = code;
        }
        // (more values than the 8-bit dictionary holds, 0.0 and 1.0029 included: the path state carries the ten floats of the shader's stack themselves, frag.glsl:136-158)
        L.niBits = !L.trans ? 0 : (niDict.size() > 256 || opt.forceNiBits8 == 2) ? 32 : ((niDict.size() <= 8 && !opt.forceNiBits8) ? 3 : 8);
        if (niDict.size() > 256) { niDict.resize(256); for (auto& m : mats) if (m.niCode > 255) m.niCode = 0; }      // (the codes are not read in that form)
        niDict.resize(std::max<size_t>(niDict.size(), 8), 0.0f);
        for (int k = 0; k < 8; k++) L.ni8[k] = niDict[k];
        // the view-dependent materials of include/pt_reproject.h: a mirror, clearcoat or transmission lobe in chooseRay (frag.glsl:745-809)
        L.matVD.assign(mats.size(), 0);
        for (int m = 0; m < nMat; m++) {
            const MatRec& r = mats[m];
            L.matVD[m] = (r.Pr != 1.0f || r.Pc != 0.0f || r.Tr > 0.0f || r.Tf[0] > 0.0f || r.illum == 5 || r.illum == 7 || r.map_Pr >= 0 || r.map_Pc >= 0 || r.map_Tr >= 0) ? 1 : 0;
        }
        L.numMat = nMat;
        return 0;
    }

    // objects / BVH: the multi-root BFS order of the inner nodes, depth-first below the top levels
    int treeOrder() {
        numObj = b.objidx[0];
        if (numObj < 0 || (size_t)numObj + 1 > b.objidx.size()) return fail("objIndices[0] exceeds the buffer");
        newIdx.assign(nNodes, -1); depth.assign(nNodes, 0); objOf.assign(nNodes, -1); seen.assign(nNodes, 0);
        std::vector<int> frontier;
        for (int o = 0; o < numObj; o++) {
            int r = b.objidx[1 + o];
            if (r < 0 || (size_t)r >= nNodes) return fail("objIndices root out of range");
            if (seen[r]) return fail("BVH node reachable twice (not a tree)");
            seen[r] = 1; frontier.push_back(r); objOf[r] = o;
        }
        {
            std::vector<int> cur = frontier, nxt;
            int d = 0;
            while (!cur.empty()) {
                nxt.clear();
                for (int n : cur) {
                    depth[n] = d;
                    if (isLeaf(n)) continue;
                    maxInnerDepth = std::max(maxInnerDepth, d);
                    newIdx[n] = (int)order.size(); order.push_back(n);
                    for (int s = 0; s < 2; s++) {
                        int ch = childOf(n, s);
                        if (ch < 0 || (size_t)ch >= nNodes) return fail("BVHtree child index out of range");
                        if (seen[ch]) return fail("BVH node reachable twice (not a tree)");
                        seen[ch] = 1; nxt.push_back(ch); objOf[ch] = objOf[n];
                    }
                }
                cur.swap(nxt); d++;
            }
        }
        // Below the top levels (the LDS tile and what every XCD's L2 keeps hot anyway) the records are laid out in depth-first order
        // instead: a node and its left child are then neighbours, and a subtree's last levels share a few cache lines — a big tree's
        // deep fetches are what misses L2.  Only the addresses change; which nodes a ray visits, and in which order, does not.
        if ((size_t)opt.bfsNodes < order.size()) {
            int cut = -1; size_t upTo = 0;                          // deepest level that is still completely inside the BFS prefix
            for (size_t k = 0; k < order.size(); k++) {
                if (k + 1 == order.size() || depth[order[k + 1]] != depth[order[k]]) {
                    if (k + 1 <= (size_t)opt.bfsNodes) { cut = depth[order[k]]; upTo = k + 1; } else break;
                }
            }
            std::vector<int> reordered(order.begin(), order.begin() + upTo), stack;
            for (size_t k = upTo; k < order.size() && depth[order[k]] == cut + 1; k++) {
                stack.assign(1, order[k]);
                while (!stack.empty()) {
                    int n = stack.back(); stack.pop_back();
                    reordered.push_back(n);
                    int Lc = childOf(n, 0), Rc = childOf(n, 1);
                    if (!isLeaf(Rc)) stack.push_back(Rc);
                    if (!isLeaf(Lc)) stack.push_back(Lc);
                }
            }
            if (reordered.size() != order.size()) return fail("internal: depth-first relayout lost nodes");
            order.swap(reordered);
            for (size_t k = 0; k < order.size(); k++) newIdx[order[k]] = (int)k;
        }
        int need = maxInnerDepth + 2;                               // worst-case entries on rayBVH's stack
        if (need > 64) return fail("BVH too deep for the reference's `int stack[64]` (frag.glsl:465)");
        L.stackDepth = std::max(need, 1);
        L.numObj = numObj; L.nInner = (int)order.size();
        return 0;
    }

    // leaf-ordered triangle records
    int triangleRecords() {
        std::vector<float4>& triRecs = L.tris;
        leafRef.assign(nNodes, REF_EMPTY);
        std::vector<int>& triObj = L.triObj;
        triObj.assign(std::max<size_t>(nTris, 1), -1);      // triangle -> object whose BVH holds it (hit.parentID of frag.glsl:573)
        for (size_t n = 0; n < nNodes; n++) {
            if (!seen[n] || !isLeaf((int)n)) continue;
            int s = toInt(b.bvhdata[8 * n + 6]), e = toInt(b.bvhdata[8 * n + 7]);
            if (e <= s) continue;                                   // empty leaf
            if (s < 0 || (size_t)e > b.leaftris.size()) return fail("leaf index range outside leafTriIndices");
            leafRef[n] = -((int)(triRecs.size() / 3) + 1);
            for (int i = s; i < e; i++) {
                int t = b.leaftris[i];
                if (t < 0 || (size_t)t >= nTris) return fail("leafTriIndices entry outside the triangle buffer");
                const float* T = b.tris.data() + 40 * (size_t)t;
                int mat = toInt(T[36]);
                if (mat < 0 || mat >= nMat) return fail("triangle material index out of range (SURVEY.md Q-14: OBJ faces before any o/g line get -1)");
                if (triObj[t] == -1) triObj[t] = objOf[n]; else if (triObj[t] != objOf[n]) { triObj[t] = -2; L.ambiguousTriObj = true; }
                uint32_t idl = (uint32_t)t | (i == e - 1 ? 0x80000000u : 0u);
                float4 rec[3]; rec[2] = f4(0, asf(idl), 0, 0);
                triRecordGeometry(T, rec);
                triRecs.insert(triRecs.end(), rec, rec + 3);
            }
        }
        L.nTriRecs = (int)(triRecs.size() / 3); L.nTris = (int)nTris;
        return 0;
    }

    void nodeRecords() {
        for (int n : order) {
            int Lc = childOf(n, 0), Rc = childOf(n, 1);
            const float* A = boxOf(Lc); const float* B = boxOf(Rc);
            float4 rec[4]; rec[3] = f4(asf((uint32_t)refOf(Lc)), asf((uint32_t)refOf(Rc)), 0, 0);
            nodeRecordBoxes(A, B, rec);
            L.nodes.insert(L.nodes.end(), rec, rec + 4);
        }
        // The hand-written intersect kernel (pt_extend_gfx950.s) reads its own node records.  80 B: the two references, then per axis (Lmin, Rmin | Lmax,
        // Rmax | Lmin, Rmin), so that a lane whose direction component is negative starts 8 B further in and receives (near pair, far pair) without a
        // min / max.  Trees that do not fit the caches pay for those bytes on every node visit (C4: 552 B per segment, the chip at 0.61 of its HBM peak):
        // they get 64-B records — references, pad, (Lmin, Rmin | Lmax, Rmax) per axis — and the kernel's min/max step (pt_set_option 19 overrides).
        const size_t nInner = order.size();
        // (what decides is whether the records the rays walk through fit an XCD's L2 beside the state stream: C4's single 100 k-node tree gains 5 % from the small
        //  records — and so do C6's 64 trees of 1.5 k nodes, 7.8 MB in all, +6.2 %, since the per-ray cull of the object loop took the 64 root tests per ray out of its
        //  vector instructions; round 4, before the cull, measured -2 % there and chose by the largest tree: profiles/r04_d_node_record_layout.txt, r05_f_*)
        const int asmStride = opt.asmNodeLayout == 0 ? 80 : opt.asmNodeLayout == 1 ? 64 : (nInner * 80 > (size_t)opt.asmNodes80Limit ? 64 : 80);
        const int W_ = asmStride / 4;
        L.nodes80.assign(std::max<size_t>(nInner, 1) * W_ + 40, 0.0f);      // (+ 160 B: developer builds of the kernel read behind a record, -DFETCH_EXTRA)
        for (size_t k = 0; k < nInner; k++) {
            const int n = order[k], Lc = childOf(n, 0), Rc = childOf(n, 1);
            const float* A = boxOf(Lc); const float* B = boxOf(Rc);
            float* o = L.nodes80.data() + (size_t)W_ * k;
            if (!node80RecordBoxes(A, B, o, asmStride)) boxesOrdered = false;
            const int lr = refOf(Lc), rr = refOf(Rc);
            std::memcpy(&o[0], &lr, 4); std::memcpy(&o[1], &rr, 4);
            if (lr == REF_EMPTY || rr == REF_EMPTY) anyEmpty = true;
        }
        L.asmNodeStride = asmStride;
    }

    void rootsAndCullGroups() {
        std::vector<ObjRoot>& roots = L.roots;
        roots.assign(std::max(numObj, 8), ObjRoot{});           // (the hand-written kernel fetches root records in batches of four: at least eight exist)
        for (int o = 0; o < numObj; o++) {
            int r = b.objidx[1 + o]; const float* A = boxOf(r);
            rootRecordBox(A, roots[o]);
            roots[o].ref = refOf(r); roots[o].pad = 0;
            // an empty root leaf would be "visited" by the reference and find nothing: it can simply never be pushed
        }
        // More than 8 BVHs: the hand-written kernel culls the object loop (frag.glsl:563-577) per ray with ONE pass over at most 64 GROUP boxes at refill
        // (pt_extend_gfx950.s, .Lmask_loop): group g = objects [g << s, (g + 1) << s), its box the union of their root boxes, appended to the root records.  A ray
        // that misses a group's box misses every root box in it (boxes of subsets; IEEE subtraction and multiplication are monotone, the ray regular: finite origin,
        // finite non-zero reciprocal direction), and a BVH whose root box the ray misses contributes nothing: rayBVH would pop the root, find neither child box hit
        // (children lie inside the root box) and return (:468-472, :521-531) — PROVIDED the root is an inner node whose child boxes lie inside an ordered root box.
        // A group holding a root that does not promise this (a leaf root: its triangles are tested whatever the box says, :478-520; foreign buffers whose children
        // stick out) gets the box (-inf, +inf): never culled.  Irregular rays skip the cull in the kernel.
        L.asmGroupShift = cullGroupShift(numObj);
        if (numObj > 8) {
            std::vector<ObjRoot> groups;
            cullGroups(numObj, opt.asmNoRootCull, [&](int o) { return boxOf(b.objidx[1 + o]); }, [&](int o) { return isLeaf(b.objidx[1 + o]); },
                       [&](int o, int side) { return boxOf(childOf(b.objidx[1 + o], side)); }, groups);
            roots.insert(roots.end(), groups.begin(), groups.end());          // at roots[numObj .. numObj + 64)
        }
    }

    void shadingRecords() {
        std::vector<float4>& shade = L.shade;
        shade.assign(std::max<size_t>(nTris, 1) * 4, float4{});
        for (size_t t = 0; t < nTris; t++) {
            shadeRecord(b.tris.data() + 40 * t, &shade[4 * t]);
        }
    }

    // ellipsoids (frag.glsl:606-611 layout)
    int ellipsoids() {
        const int nE = toInt(b.ellip[0]);
        if (nE < 0 || b.ellip.size() < (size_t)1 + 11 * (size_t)nE) return fail("EllipData shorter than its count says");
        L.ellip.resize(std::max(nE, 1));
        const size_t N = (size_t)nE;
        for (size_t i = 0; i < N; i++) {
            EllipRec& r = L.ellip[i];
            ellipRecord(b.ellip.data(), N, i, r);
            if (r.mat < 0 || r.mat >= nMat) return fail("ellipsoid material index out of range");
            if (L.mats[r.mat].hasMaps) L.ellipMaps = true;           // sampled at the uv of the closest triangle found before the ellipsoid (frag.glsl:574 vs :619-630): State::HX
        }
        L.numEllip = nE;
        return 0;
    }

    // textures stay the RGBA8 texels the caller uploaded (dispatch.java:349-354: GL_RGBA8); byte / 255.0f happens at fetch (unorm8, pt_device.hpp).
    // The texture table beyond the sky: ONE block for all textures
    void textures() {
        const size_t n = std::max<size_t>(b.textures.size(), 1);
        L.texOff.assign(n, 0); L.texW.assign(n, 0); L.texH.assign(n, 0);
        L.texW[0] = b.skyW; L.texH[0] = b.skyH;
        for (size_t ti = 1; ti < b.textures.size(); ti++) {
            const SceneBuffers::HostTex& T = b.textures[ti];
            L.texW[ti] = T.w; L.texH[ti] = T.h;
            if (T.rgba.empty()) continue;
            L.texOff[ti] = L.texels.size() / 4;
            L.texels.insert(L.texels.end(), T.rgba.begin(), T.rgba.begin() + (size_t)T.w * T.h * 4);
        }
    }

    void modes() {
        // LDS tile: as many leading (top-of-tree) node records and triangle records as the budget allows
        int budget = opt.ldsBudget - L.stackDepth * EXTEND_BLOCK * 4;
        int ln = 0, lt = 0;
        if (budget > 0) {
            ln = std::min(L.nInner, budget / 64);
            int rest = budget - ln * 64;
            lt = std::min(L.nTriRecs, rest / 48);
            if (ln < L.nInner) lt = std::min(lt, 0);               // triangles only once every node fits
        }
        L.ldsNodes = ln; L.ldsTris = lt;
        // persistent kernel: one staged tile per resident block
        L.stackMode = (L.nInner < 32767 && L.nTriRecs < 32767) ? 0 : (L.nInner <= 131071 && L.nTriRecs <= 131071 && L.stackDepth <= 32) ? 1 : 2;
        if (opt.stackModeForce >= 0) L.stackMode = std::max(L.stackMode, opt.stackModeForce);      // only ever towards wider entries
        {
            int cb = opt.extendCacheBytes;
            int pn = std::min(L.nInner, cb / 64);
            int pt_ = (pn == L.nInner) ? std::min(L.nTriRecs, (cb - pn * 64) / 48) : 0;
            L.pLdsNodes = pn; L.pLdsTris = pt_;
        }
        // which scenes the hand-written kernel takes (the others run on the compiled k_extend_persist, same results)
        for (int o = 0; o < numObj; o++) if (L.roots[o].ref == REF_EMPTY) anyEmpty = true;
        L.asmWhyNot.clear();
        if (numObj < 1 || numObj > 1024) L.asmWhyNot = "no BVH or more than 1024";
        else if (anyEmpty) L.asmWhyNot = "a leaf without triangles";
        else if (!boxesOrdered && L.asmNodeStride == 80) L.asmWhyNot = "a node box with min > max or a NaN";      // (the 64-B records' min/max step is rayBox as written)
        else if (L.tris.size() / 3 >= (1u << 23) - 1 || order.size() >= (1u << 23) - 1) L.asmWhyNot = "more than 2^23 - 2 inner nodes or triangle records (24-bit stack entries)";
        L.asmEligible = L.asmWhyNot.empty();
    }
};

// Validates the reference's buffers and builds the device-private layout (see pt_device.hpp).  0, or PT_ERR_SCENE with the reason in err; out is
// meaningful only after 0.  runLayout: the steps on a run the caller keeps (pt_scene_move.hpp reads the order it decided)
inline int runLayout(LayoutRun& r) {
    int rc;
    if ((rc = r.presence()) || (rc = r.materials()) || (rc = r.treeOrder()) || (rc = r.triangleRecords())) return rc;
    r.nodeRecords();
    r.rootsAndCullGroups();
    r.shadingRecords();
    if ((rc = r.ellipsoids())) return rc;
    r.textures();
    r.modes();
    return 0;
}
inline int layoutScene(const SceneBuffers& in, const LayoutOptions& opt, SceneLayout& out, std::string& err) {
    out = SceneLayout{};
    LayoutRun r(in, opt, out, err);
    return runLayout(r);
}

}  // namespace ptl
