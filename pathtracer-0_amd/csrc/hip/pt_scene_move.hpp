// pt_scene_move.hpp — the host-only half of the in-place move of a scene's triangles (include/pt_move.h): what of a built layout depends on the
// coordinates of binding 3 and the boxes of binding 10, and how to rewrite exactly that.  Plain C++: no HIP runtime call and no context.
//
//   MoveMap     what a patch needs beyond what the records already hold: per inner record, in the layout's final order, the node ids of its two
//               children; per object its root; the modes of the layout that decide whether a patch can promise equality.  It is read off the
//               LayoutRun that decided the order (treeOrder of pt_scene_layout.hpp), never from a traversal of its own.
//   applyMove   the CPU statement of the patch, through the per-record functions layoutScene itself calls.  The kernels of pt_move.hip do to the
//               device arrays what this does to a SceneLayout; tests/c/scene_move_check.cpp holds it to layoutScene on the moved buffers.
//
// Triangle ids need no map: triangle record i carries its id in the low 31 bits of float 9, which the patch keeps (with the last-in-leaf bit).
// The root records keep their references; the map names the root nodes.
#pragma once
#include "pt_scene_layout.hpp"

namespace ptl {

struct MoveMap {
    std::vector<int32_t> child;                      // 2 per inner record k: the node ids (rows of binding 10) of its left and right child
    std::vector<int32_t> rootNode, rootRef;          // per object: its root's node id, and the reference its root record holds
    std::vector<char> rootLeaf;                      // per object: the root is a leaf
    int nInner = 0, numObj = 0, nRows = 0;           // nRows: rows of binding 10 the ids stay below
    int asmStride = 80, asmGroupShift = 0;
    bool asmNoRootCull = false, boxesOrdered = true, anyEmpty = false;
    // The patch cannot promise what layoutScene would decide: the built layout had an unordered box in 80-byte records and no empty leaf, so it was
    // not eligible for the hand-written kernel; refit boxes of non-empty leaves are always ordered, so a layout of the new buffers would be.
    bool needsRebuild() const { return !boxesOrdered && asmStride == 80 && !anyEmpty; }
};

// The order-dependent part of the map from a run whose treeOrder() has succeeded (triangleRecords() too when the references are wanted)
inline void orderOf(const LayoutRun& r, MoveMap& m) {
    m.nInner = (int)r.order.size(); m.numObj = r.numObj; m.nRows = (int)(r.b.bvhdata.size() / 8);
    m.child.resize(2 * r.order.size());
    for (size_t k = 0; k < r.order.size(); k++) { m.child[2 * k] = r.childOf(r.order[k], 0); m.child[2 * k + 1] = r.childOf(r.order[k], 1); }
    m.rootNode.resize(r.numObj); m.rootRef.assign(r.numObj, 0); m.rootLeaf.resize(r.numObj);
    for (int o = 0; o < r.numObj; o++) {
        const int n = r.b.objidx[1 + o];
        m.rootNode[o] = n; m.rootLeaf[o] = r.isLeaf(n);
        // (an inner root's reference is its record's index, which the order decides; a leaf root's comes from triangleRecords, where that has run)
        m.rootRef[o] = !m.rootLeaf[o] ? r.newIdx[n] : !r.leafRef.empty() ? r.leafRef[n] : 0;
    }
    m.asmGroupShift = cullGroupShift(r.numObj);
    m.asmNoRootCull = r.opt.asmNoRootCull;
}

// layoutScene and the map of what it built, from the one run
inline int layoutSceneWithMap(const SceneBuffers& in, const LayoutOptions& opt, SceneLayout& out, MoveMap& map, std::string& err) {
    out = SceneLayout{};
    LayoutRun r(in, opt, out, err);
    if (const int rc = runLayout(r)) return rc;
    map = MoveMap{};
    orderOf(r, map);
    map.asmStride = out.asmNodeStride; map.boxesOrdered = r.boxesOrdered; map.anyEmpty = r.anyEmpty;
    return 0;
}

// The order alone, for a scene that layoutScene has accepted: the tree walk and nothing else (no record is built).  The modes are the caller's to
// fill in from what it built.
inline int moveMapOrder(const SceneBuffers& in, const LayoutOptions& opt, MoveMap& map, std::string& err) {
    SceneLayout scratch;
    LayoutRun r(in, opt, scratch, err);
    r.nTris = in.tris.size() / 40; r.nNodes = in.bvhtree.size() / 3;
    if (in.objidx.empty() || in.bvhdata.size() < 8 * r.nNodes) return r.fail("internal: moveMapOrder on a scene that was not laid out");
    if (const int rc = r.treeOrder()) return rc;
    map = MoveMap{};
    orderOf(r, map);
    return 0;
}

// The root boxes and, beyond 8 objects, the 64 group boxes of `roots` (numObj, at least 8, records, then the groups) from the rows of binding 10;
// references and padding of the root records stay
// (root(o): object o's root row; child(o, side): the row of a child of an inner root.  Asked for nothing else)
template <class Root, class Child>
inline void moveRootsFrom(const MoveMap& m, Root root, Child child, ObjRoot* roots) {
    for (int o = 0; o < m.numObj; o++) rootRecordBox(root(o), roots[o]);
    if (m.numObj <= 8) return;
    std::vector<ObjRoot> groups;
    cullGroups(m.numObj, m.asmNoRootCull, root, [&](int o) { return m.rootLeaf[o] != 0; }, child, groups);
    std::copy(groups.begin(), groups.end(), roots + std::max(m.numObj, 8));
}
inline void moveRoots(const MoveMap& m, const float* bvhdata, ObjRoot* roots) {
    moveRootsFrom(m, [&](int o) { return bvhdata + 8 * (size_t)m.rootNode[o]; },
                  [&](int o, int side) { return bvhdata + 8 * (size_t)m.child[2 * (size_t)m.rootRef[o] + side]; }, roots);
}
// The same from gathered rows (include/pt_pose.h): three per object — its root's, then, of an inner root, its two children's — whose node ids
// moveRowIds lists (a leaf root's two spare entries name the root again: never read)
inline void moveRowIds(const MoveMap& m, std::vector<int32_t>& ids) {
    ids.resize(3 * (size_t)m.numObj);
    for (int o = 0; o < m.numObj; o++) {
        ids[3 * (size_t)o] = m.rootNode[o];
        for (int side = 0; side < 2; side++) ids[3 * (size_t)o + 1 + side] = m.rootLeaf[o] ? m.rootNode[o] : m.child[2 * (size_t)m.rootRef[o] + side];
    }
}
inline void moveRootsGathered(const MoveMap& m, const float* rows, ObjRoot* roots) {
    moveRootsFrom(m, [&](int o) { return rows + 24 * (size_t)o; }, [&](int o, int side) { return rows + 24 * (size_t)o + 8 * (size_t)(1 + side); }, roots);
}

// What binding 7 must keep for a patch: the count and every material index (ellipMaps could change otherwise).  Both buffers were or are checked
// by ellipsoidsUsable.
inline bool ellipPatchable(const std::vector<float>& was, const float* now, size_t nowFloats) {
    if (was.empty() || nowFloats < 1) return false;
    const int nOld = toInt(was[0]), nNew = toInt(now[0]);
    if (nOld != nNew || nNew < 0) return false;
    const size_t N = (size_t)nNew;
    if (was.size() < 1 + 11 * N || nowFloats < 1 + 11 * N) return false;
    for (size_t i = 0; i < N; i++) if (toInt(was[1 + N * 10 + i]) != toInt(now[1 + N * 10 + i])) return false;
    return true;
}
// the ellipsoids() refusals of layoutScene on a new binding 7, with its texts; 0 or PT_ERR_SCENE
inline int ellipsoidsUsable(const float* E, size_t nFloats, int nMat, std::string& err) {
    if (nFloats < 1) { err = "EllipData (binding 7) not set"; return PT_ERR_SCENE; }
    const int nE = toInt(E[0]);
    if (nE < 0 || nFloats < (size_t)1 + 11 * (size_t)nE) { err = "EllipData shorter than its count says"; return PT_ERR_SCENE; }
    for (size_t i = 0; i < (size_t)nE; i++) {
        const int mat = toInt(E[1 + (size_t)nE * 10 + i]);
        if (mat < 0 || mat >= nMat) { err = "ellipsoid material index out of range"; return PT_ERR_SCENE; }
    }
    return 0;
}
inline void moveEllipsoids(const float* E, std::vector<EllipRec>& recs) {
    const size_t N = (size_t)toInt(E[0]);
    for (size_t i = 0; i < N; i++) ellipRecord(E, N, i, recs[i]);
}

// THE PATCH.  L: layoutScene of the old buffers; m: its map, !m.needsRebuild(); tris: the new binding 3 (as many triangles as before); bvhdata: the
// refit binding 10; ellip: the new binding 7 (ellipPatchable against the old one) or null.  Afterwards L is layoutScene of the new buffers, byte for
// byte.  Returns whether every node box it wrote is ordered (what layoutScene would have found: the caller holds it against what the modes assume).
inline bool applyMove(SceneLayout& L, const MoveMap& m, const float* tris, const float* bvhdata, const float* ellip) {
    // triangle records: floats 0-8; float 9 (id, last-in-leaf bit) and the padding stay
    for (int i = 0; i < L.nTriRecs; i++) {
        float4* rec = &L.tris[3 * (size_t)i];
        uint32_t idl; std::memcpy(&idl, &rec[2].y, 4);
        triRecordGeometry(tris + 40 * (size_t)(idl & 0x7fffffffu), rec);
    }
    // shading records, by triangle id: every triangle, referenced or not
    for (int t = 0; t < L.nTris; t++) shadeRecord(tris + 40 * (size_t)t, &L.shade[4 * (size_t)t]);
    // node records: the boxes of both forms; references and padding stay
    bool ordered = true;
    const int W_ = L.asmNodeStride / 4;
    for (int k = 0; k < m.nInner; k++) {
        const float* A = bvhdata + 8 * (size_t)m.child[2 * (size_t)k]; const float* B = bvhdata + 8 * (size_t)m.child[2 * (size_t)k + 1];
        nodeRecordBoxes(A, B, &L.nodes[4 * (size_t)k]);
        if (!node80RecordBoxes(A, B, L.nodes80.data() + (size_t)W_ * k, L.asmNodeStride)) ordered = false;
    }
    moveRoots(m, bvhdata, L.roots.data());
    if (ellip) moveEllipsoids(ellip, L.ellip);
    return ordered;
}

}  // namespace ptl
