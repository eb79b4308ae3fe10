// scene_move_check.cpp — holds applyMove (csrc/hip/pt_scene_move.hpp), the CPU statement of the in-place move of include/pt_move.h, to layoutScene
// on the moved buffers: every array byte for byte, every count and mode (tests/test_scene_move.py builds it with g++ under the host sanitizers).
//
//   scene_move_check SCENE MOVE
// SCENE: the file scene_layout_check.cpp reads (bindings, textures, eight options).  MOVE, little-endian: u64 count and the floats of the new
// binding 3, of the new binding 10, of the new binding 7 (count 0: binding 7 stays).
// Prints rc / err of the old layout; `slow 1` when the map says the patch cannot promise equality (applyMove is then not called); else what
// differs between the patched layout and layoutScene(new buffers) (`differs` is empty when nothing does), whether the order-only map of the
// runtime equals the full run's, whether applyMove's ordered flag is what the new layout found, and the topology digests of both buffer sets.
#include "../../pathtracer-0_amd/csrc/hip/pt_scene_move.hpp"
#include "../../pathtracer-0_amd/csrc/hip/pt_refit_plan.hpp"

#include <cstdio>
#include <cstdlib>

namespace {

using namespace ptl;

void need(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "input file: %s\n", what); std::exit(2); } }
template <typename T> T rd(FILE* f) { T v; need(std::fread(&v, sizeof(T), 1, f) == 1, "truncated"); return v; }
template <typename T> void rdVec(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); need(n == 0 || std::fread(v.data(), sizeof(T), n, f) == n, "truncated"); }

void readScene(const char* path, SceneBuffers& b, LayoutOptions& o) {
    FILE* f = std::fopen(path, "rb");
    need(f != nullptr, "cannot open");
    for (uint32_t k = rd<uint32_t>(f); k > 0; k--) {
        const int32_t id = rd<int32_t>(f); const size_t n = (size_t)rd<uint64_t>(f);
        switch (id) {
            case PT_BIND_ORIGIN: rdVec(f, b.origin, n); break;
            case PT_BIND_ROTATION: rdVec(f, b.rotation, n); break;
            case PT_BIND_MOUSE: rdVec(f, b.mouse, n); break;
            case PT_BIND_TRIANGLES: rdVec(f, b.tris, n); break;
            case PT_BIND_PARAMS: rdVec(f, b.params, n); break;
            case PT_BIND_IMPLICITS: rdVec(f, b.imp, n); break;
            case PT_BIND_ELLIPSOIDS: rdVec(f, b.ellip, n); break;
            case PT_BIND_BVHDATA: rdVec(f, b.bvhdata, n); break;
            case PT_BIND_BVHTREE: rdVec(f, b.bvhtree, n); break;
            case PT_BIND_LEAFTRIS: rdVec(f, b.leaftris, n); break;
            case PT_BIND_OBJINDICES: rdVec(f, b.objidx, n); break;
            case PT_BIND_MATERIALS: rdVec(f, b.mtl, n); break;
            default: need(false, "unknown binding");
        }
    }
    for (uint32_t k = rd<uint32_t>(f); k > 0; k--) {
        const int32_t index = rd<int32_t>(f), w = rd<int32_t>(f), h = rd<int32_t>(f);
        need(index >= 0 && index <= 4095 && w >= 1 && h >= 1, "bad texture");
        if ((size_t)index >= b.textures.size()) b.textures.resize((size_t)index + 1);
        SceneBuffers::HostTex& T = b.textures[index];
        rdVec(f, T.rgba, (size_t)w * h * 4); T.w = w; T.h = h;
        if (index == 0) { b.sky = T.rgba; b.skyW = w; b.skyH = h; }
    }
    o.bfsNodes = rd<int32_t>(f); o.asmNodeLayout = rd<int32_t>(f); o.asmNoRootCull = rd<int32_t>(f) != 0; o.forceNiBits8 = rd<int32_t>(f);
    o.ldsBudget = rd<int32_t>(f); o.extendCacheBytes = rd<int32_t>(f); o.stackModeForce = rd<int32_t>(f); o.asmNodes80Limit = rd<int32_t>(f);
    std::fclose(f);
}

std::string differs;
template <typename T> void same(const char* name, const std::vector<T>& a, const std::vector<T>& b) {
    if (a.size() != b.size() || (a.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) != 0)) differs += std::string(" ") + name;
}
template <typename T> void sameValue(const char* name, const T& a, const T& b) { if (!(a == b)) differs += std::string(" ") + name; }

uint64_t digestOf(const SceneBuffers& b) {
    return ptr::topologyDigest(b.bvhtree.data(), b.bvhtree.size(), b.leaftris.data(), b.leaftris.size(), b.objidx.data(), b.objidx.size(), b.bvhdata.data(),
                               b.bvhdata.size());
}

}  // namespace

int main(int argc, char** argv) {
    need(argc == 3, "usage: scene_move_check SCENE MOVE");
    SceneBuffers old; LayoutOptions o;
    readScene(argv[1], old, o);
    std::vector<float> tris, data, ellip;
    {
        FILE* f = std::fopen(argv[2], "rb");
        need(f != nullptr, "cannot open");
        rdVec(f, tris, (size_t)rd<uint64_t>(f)); rdVec(f, data, (size_t)rd<uint64_t>(f)); rdVec(f, ellip, (size_t)rd<uint64_t>(f));
        std::fclose(f);
    }
    need(tris.size() == old.tris.size() && data.size() == old.bvhdata.size(), "the move changes a buffer's length");

    SceneLayout L; MoveMap map; std::string err;
    const int rc = layoutSceneWithMap(old, o, L, map, err);
    std::printf("rc %d\nerr %s\n", rc, err.c_str());
    if (rc) return 0;
    std::printf("slow %d\n", map.needsRebuild() ? 1 : 0);
    std::printf("nInner %d\nnumObj %d\nasmStride %d\nasmGroupShift %d\nboxesOrdered %d\nanyEmpty %d\n", map.nInner, map.numObj, map.asmStride, map.asmGroupShift,
                map.boxesOrdered, map.anyEmpty);
    // the order-only map of the runtime names the same children and roots
    MoveMap lean;
    const int rcLean = moveMapOrder(old, o, lean, err);
    bool leanSame = rcLean == 0 && lean.child == map.child && lean.rootNode == map.rootNode && lean.rootLeaf == map.rootLeaf && lean.nInner == map.nInner &&
                    lean.numObj == map.numObj && lean.nRows == map.nRows && lean.asmGroupShift == map.asmGroupShift && lean.asmNoRootCull == map.asmNoRootCull;
    for (int ob = 0; leanSame && ob < map.numObj; ob++) if (!map.rootLeaf[ob] && lean.rootRef[ob] != map.rootRef[ob]) leanSame = false;
    std::printf("order_same %d\n", leanSame ? 1 : 0);
    for (int32_t c : map.child) need(c >= 0 && c < map.nRows, "a child id outside binding 10");
    if (map.needsRebuild()) return 0;

    const bool patchEllip = !ellip.empty();
    if (patchEllip) {
        const int erc = ellipsoidsUsable(ellip.data(), ellip.size(), L.numMat, err);
        std::printf("ellip_rc %d\nellip_patchable %d\n", erc, erc == 0 && ellipPatchable(old.ellip, ellip.data(), ellip.size()) ? 1 : 0);
        if (erc || !ellipPatchable(old.ellip, ellip.data(), ellip.size())) return 0;
    }
    const bool ordered = applyMove(L, map, tris.data(), data.data(), patchEllip ? ellip.data() : nullptr);

    SceneBuffers now = old;
    now.tris = tris; now.bvhdata = data;
    if (patchEllip) now.ellip = ellip;
    SceneLayout N; MoveMap mapN;
    const int rcN = layoutSceneWithMap(now, o, N, mapN, err);
    std::printf("new_rc %d\nnew_err %s\n", rcN, err.c_str());
    if (rcN) return 0;
    same("nodes", L.nodes, N.nodes); same("nodes80", L.nodes80, N.nodes80); same("tris", L.tris, N.tris); same("shade", L.shade, N.shade);
    same("triObj", L.triObj, N.triObj); same("roots", L.roots, N.roots); same("ellip", L.ellip, N.ellip); same("mats", L.mats, N.mats);
    same("matVD", L.matVD, N.matVD); same("niDict", L.niDict, N.niDict); same("texels", L.texels, N.texels); same("texOff", L.texOff, N.texOff);
    same("texW", L.texW, N.texW); same("texH", L.texH, N.texH);
    same("ni8", std::vector<float>(L.ni8, L.ni8 + 8), std::vector<float>(N.ni8, N.ni8 + 8));
    sameValue("nInner", L.nInner, N.nInner); sameValue("nTriRecs", L.nTriRecs, N.nTriRecs); sameValue("nTris", L.nTris, N.nTris);
    sameValue("numObj", L.numObj, N.numObj); sameValue("numEllip", L.numEllip, N.numEllip); sameValue("numMat", L.numMat, N.numMat);
    sameValue("trans", L.trans, N.trans); sameValue("anySubsurface", L.anySubsurface, N.anySubsurface); sameValue("anyMaps", L.anyMaps, N.anyMaps);
    sameValue("ellipMaps", L.ellipMaps, N.ellipMaps); sameValue("ambiguousTriObj", L.ambiguousTriObj, N.ambiguousTriObj); sameValue("niBits", L.niBits, N.niBits);
    sameValue("stackDepth", L.stackDepth, N.stackDepth); sameValue("asmNodeStride", L.asmNodeStride, N.asmNodeStride);
    sameValue("asmGroupShift", L.asmGroupShift, N.asmGroupShift); sameValue("ldsNodes", L.ldsNodes, N.ldsNodes); sameValue("ldsTris", L.ldsTris, N.ldsTris);
    sameValue("stackMode", L.stackMode, N.stackMode); sameValue("pLdsNodes", L.pLdsNodes, N.pLdsNodes); sameValue("pLdsTris", L.pLdsTris, N.pLdsTris);
    sameValue("asmEligible", L.asmEligible, N.asmEligible); sameValue("asmWhyNot", L.asmWhyNot, N.asmWhyNot);
    sameValue("map.child", map.child, mapN.child); sameValue("map.rootRef", map.rootRef, mapN.rootRef); sameValue("map.anyEmpty", map.anyEmpty, mapN.anyEmpty);
    std::printf("differs%s\n", differs.c_str());
    std::printf("ordered_as_found %d\n", ordered == mapN.boxesOrdered ? 1 : 0);
    std::printf("asmWhyNot %s\n", N.asmWhyNot.c_str());
    std::printf("group_pads");
    for (size_t g = 0; L.numObj > 8 && g < 64; g++) std::printf(" %d", L.roots[std::max(L.numObj, 8) + g].pad);
    std::printf("\n");
    std::printf("tri_nan %d\n", [&] { int n = 0; for (const float4& v : L.tris) n += (v.x != v.x) + (v.y != v.y) + (v.w != v.w); return n; }());
    std::printf("digest_old %016llx\ndigest_new %016llx\n", (unsigned long long)digestOf(old), (unsigned long long)digestOf(now));
    return 0;
}
