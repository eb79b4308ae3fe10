// scene_layout_check.cpp — runs layoutScene (csrc/hip/pt_scene_layout.hpp) on the CPU over a scene file and prints what it decided and built: the
// return code, the error text, every scalar of SceneLayout, and a 64-bit FNV-1a digest with the byte length of every array
// (tests/test_scene_layout.py builds it with g++, once plain and once under the host sanitizers).
//
// The file, little-endian:  u32 bindings, then per binding  i32 id (PT_BIND_*), u64 count of 4-byte elements, the elements;
//                           u32 textures, then per texture  i32 index, i32 w, i32 h, w*h*4 bytes (as pt_set_texture takes them: index 0 is the sky);
//                           8 x i32  bfsNodes, asmNodeLayout, asmNoRootCull, forceNiBits8, ldsBudget, extendCacheBytes, stackModeForce, asmNodes80Limit.
#include "../../pathtracer-0_amd/csrc/hip/pt_scene_layout.hpp"

#include <cstdio>
#include <cstdlib>

namespace {

using namespace ptl;

void need(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "scene file: %s\n", what); std::exit(2); } }
template <typename T> T rd(FILE* f) { T v; need(std::fread(&v, sizeof(T), 1, f) == 1, "truncated"); return v; }
template <typename T> void rdVec(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); need(n == 0 || std::fread(v.data(), sizeof(T), n, f) == n, "truncated"); }

template <typename T> void digest(const char* name, const std::vector<T>& v) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    const size_t n = v.size() * sizeof(T);
    for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; }
    std::printf("%s %016llx %zu\n", name, (unsigned long long)h, n);
}

}  // namespace

int main(int argc, char** argv) {
    need(argc == 2, "usage: scene_layout_check FILE");
    FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open");
    SceneBuffers b;
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
    LayoutOptions o;
    o.bfsNodes = rd<int32_t>(f); o.asmNodeLayout = rd<int32_t>(f); o.asmNoRootCull = rd<int32_t>(f) != 0; o.forceNiBits8 = rd<int32_t>(f);
    o.ldsBudget = rd<int32_t>(f); o.extendCacheBytes = rd<int32_t>(f); o.stackModeForce = rd<int32_t>(f); o.asmNodes80Limit = rd<int32_t>(f);
    std::fclose(f);

    SceneLayout L; std::string err;
    const int rc = layoutScene(b, o, L, err);
    std::printf("rc %d\nerr %s\n", rc, err.c_str());
    if (rc) return 0;
    std::printf("nInner %d\nnTriRecs %d\nnTris %d\nnumObj %d\nnumEllip %d\nnumMat %d\n", L.nInner, L.nTriRecs, L.nTris, L.numObj, L.numEllip, L.numMat);
    std::printf("trans %d\nanySubsurface %d\nanyMaps %d\nellipMaps %d\nambiguousTriObj %d\n", L.trans, L.anySubsurface, L.anyMaps, L.ellipMaps, L.ambiguousTriObj);
    std::printf("niBits %d\nstackDepth %d\nasmNodeStride %d\nasmGroupShift %d\nldsNodes %d\nldsTris %d\nstackMode %d\npLdsNodes %d\npLdsTris %d\n", L.niBits, L.stackDepth,
                L.asmNodeStride, L.asmGroupShift, L.ldsNodes, L.ldsTris, L.stackMode, L.pLdsNodes, L.pLdsTris);
    std::printf("asmEligible %d\nasmWhyNot %s\n", L.asmEligible, L.asmWhyNot.c_str());
    digest("ni8", std::vector<float>(L.ni8, L.ni8 + 8));
    digest("nodes", L.nodes); digest("nodes80", L.nodes80); digest("tris", L.tris); digest("shade", L.shade); digest("triObj", L.triObj);
    digest("roots", L.roots); digest("ellip", L.ellip); digest("mats", L.mats); digest("matVD", L.matVD); digest("niDict", L.niDict);
    digest("texels", L.texels);
    digest("texOff", std::vector<uint64_t>(L.texOff.begin(), L.texOff.end())); digest("texW", L.texW); digest("texH", L.texH);
    return 0;
}
