"""The scenes the refit tests share (tests/test_refit_model.py, tests/test_refit_plan.py, tests/test_gpu_refit.py): {name: buffers}, every tree built
by the CPU builder.  Built once per process."""
import numpy as np

from test_gpu_parity import _soup_obj

# (n, degenerate, seed): the first five are rows of test_gpu_bvh_builder_random_soups; 128, 129 and 257 put leaf and node counts around a 256-lane block
SOUPS = [(2, 0.0, 1), (3, 0.0, 2), (64, 0.5, 4), (65, 0.0, 3), (1000, 0.0, 5), (128, 0.0, 8), (129, 0.0, 9), (257, 0.0, 10)]
WORKLOADS = {"C1": {}, "C2": {}, "C3": dict(subdiv=1), "C4": dict(nu=12, nv=10), "C5": dict(subdiv=1), "C6": dict(nu=8, nv=8), "T1": {}, "M1": {}}
_CACHE = {}


def soup(pt, n, degenerate, seed, scale=1.0):
    """two objects of the same soup, the second shifted by 2 (times the scale, so that a power-of-two scale gives the exact image of the unscaled
    scene): ids and leaf offsets continue"""
    text = _soup_obj(np.random.RandomState(seed), n, degenerate)
    sc = pt.hostlib.Scene(); sc.addMaterial("m")
    sc.addObjectText(text, 0, scale=scale)
    sc.addObjectText(text, 0, scale=scale, shift=(2.0 * scale, 0.0, 0.0))
    return sc.pack()


def ladder_text(count=330):
    """test_gpu_bvh_builder_deep_unbalanced_tree's triangles: the tree runs into the builder's depth limit of 256"""
    lines, k = ["o ladder", "vn 0 0 1"], 0
    for i in range(count):
        x, h = 2.0 ** (-3 * i), 2.0 ** (-3 * i - 3)
        for (dx, dy) in ((0.0, 0.0), (h, 0.0), (0.0, h)):
            lines.append("v %.17g %.17g 0" % (x + dx, dy))
        lines.append("f %d//1 %d//1 %d//1" % (k + 1, k + 2, k + 3))
        k += 3
    return "\n".join(lines) + "\n"


def ladder(pt):
    sc = pt.hostlib.Scene(); sc.addMaterial("m")
    sc.addObjectText(ladder_text(), 0)
    return sc.pack()


def chain(heights=256, seed=31):
    """a hand-made ladder of exactly `heights` heights in the reference's pre-order numbering: inner node 2k has the leaf 2k + 1 on its left and the
    next inner node on its right; the last pair are two leaves.  One random triangle per leaf, in a shuffled leaf order; the boxes are stale zeros."""
    rs = np.random.RandomState(seed)
    n_leaves, n = heights + 1, 2 * heights + 1
    tree = np.full((n, 3), -1, np.int32)
    tree[:, 0] = np.arange(n)
    data = np.zeros((n, 8), np.float32)
    leaf = rs.permutation(n_leaves).astype(np.int32)
    k = 0
    for i in range(0, n - 1, 2):
        tree[i, 1:] = (i + 1, i + 2)
    for i in range(n):
        if tree[i, 1] == -1:
            data[i, 6:8] = (k, k + 1)
            k += 1
    assert k == n_leaves
    tris = np.zeros((n_leaves, 40), np.float32)
    for c in (0, 4, 8):
        tris[:, c:c + 3] = rs.rand(n_leaves, 3)
    return {3: tris.reshape(-1), 10: data.reshape(-1), 11: tree.reshape(-1), 12: leaf, 13: np.array([1, 0], np.int32)}


def objects_and_loose(pt):
    """two objects with loose addTri triangles before, between and after them: triangles no tree references"""
    sc = pt.hostlib.Scene(); sc.addMaterial("m")
    sc.addTri((5, 5, 5), (6, 5, 5), (5, 6, 5), 0)
    sc.addObjectText(_soup_obj(np.random.RandomState(21), 40, 0.0), 0)
    sc.addTri((-5, -5, -5), (-6, -5, -5), (-5, -6, -5), 0)
    sc.addObjectText(_soup_obj(np.random.RandomState(22), 17, 0.2), 0, shift=(0.0, 3.0, 0.0))
    sc.addTri((7, 7, 7), (8, 7, 7), (7, 8, 7), 0)
    return sc.pack()


def workload(pt, name):
    return pt.scenes.build(name, 96, 54, **WORKLOADS[name])


def extra(pt):
    """{name: buffers} of the soups, the ladder and the scene with loose triangles (built by the CPU builder: their binding 10 is the reference's),
    and of the hand-made chain of 256 heights (its binding 10 is stale)"""
    if "extra" not in _CACHE:
        out = {f"soup{n}": soup(pt, n, d, s) for n, d, s in SOUPS}
        out["ladder"] = ladder(pt)
        out["loose"] = objects_and_loose(pt)
        out["chain256"] = chain()
        _CACHE["extra"] = out
    return _CACHE["extra"]


def workloads(pt):
    if "workloads" not in _CACHE:
        _CACHE["workloads"] = {name: workload(pt, name).buffers for name in WORKLOADS}
    return _CACHE["workloads"]


def perturbed(tris, seed, amount=0.05):
    """binding 3 with every vertex moved a little: a deformation, the topology's triangle ids unchanged"""
    t = np.array(tris, np.float32).reshape(-1, 40)
    rs = np.random.RandomState(seed)
    for c in (0, 4, 8):
        t[:, c:c + 3] += (rs.randn(len(t), 3) * amount).astype(np.float32)
    return t.reshape(-1)
