"""The scenes and moves the tests of include/pt_move.h share (tests/test_scene_move.py on the CPU, tests/test_gpu_move.py on the GPU): complete
scenes (every binding the layout step asks for, a sky) around the buffers of tests/_refit_cases.py, the hand-made ones, and for each the moved
binding 3 with the binding 10 that tests/_refit_model.py refits to it.  Built once per process."""
import numpy as np

import _refit_cases as RC
import _refit_model as RM
from test_gpu_parity import _soup_obj
from test_scene_layout import edit, hand_scene, material, materials

f32 = np.float32
W, H = 48, 27
_CACHE = {}


def complete(pt, b, cam=(1.5, 0.5, -4.0)):
    """buffers of Scene.pack() (or fewer) -> every binding of a renderable scene at W x H, 2 samples, 3 bounces"""
    b = dict(b)
    b.setdefault(5, np.array([0.0], f32)); b.setdefault(7, np.array([0.0], f32)); b.setdefault(14, materials(material()))
    b[0] = np.array(cam, f32); b[1] = np.zeros(3, f32); b[2] = np.array([-1e6, -1e6, 0], f32)
    b[4] = pt.scenes.make_params(W, H, 2, 3)
    return b


SKY = {0: np.full((1, 1, 4), 200, np.uint8)}


def many_objects(pt, n=70, tris=12):
    """more than 64 objects, each an inner root over a small soup: asmGroupShift >= 1, two objects per group box"""
    sc = pt.hostlib.Scene(); sc.addMaterial("m")
    for k in range(n):
        sc.addObjectText(_soup_obj(np.random.RandomState(100 + k), tris, 0.0), 0, shift=(1.5 * (k % 10), 1.5 * (k // 10), 0.0))
    return sc.pack()


def with_leaf_root(pt, n=10):
    """more than 8 objects (group boxes exist); the last object is one hand-made triangle under a leaf root (the builder makes none), so its group
    box must stay infinite"""
    sc = pt.hostlib.Scene(); sc.addMaterial("m")
    for k in range(n - 1):
        sc.addObjectText(_soup_obj(np.random.RandomState(200 + k), 9, 0.0), 0, shift=(1.5 * k, 0.0, 0.0))
    b = sc.pack()
    nt, nn, nl = b[3].size // 40, b[11].size // 3, b[12].size
    t = np.zeros(40, f32)
    x = 1.5 * (n - 1)
    t[0:3] = (x, 0, 0); t[4:7] = (x + 1, 0, 0); t[8:11] = (x, 1, 0); t[14] = 1.0; t[18] = 1.0; t[34] = 1.0      # (the three normals: +z)
    b[3] = np.concatenate([b[3], t])
    b[10] = np.concatenate([b[10], np.array([x, 0, 0, x + 1, 1, 0, nl, nl + 1], f32)])
    b[11] = np.concatenate([b[11], np.array([nn, -1, -1], np.int32)])
    b[12] = np.concatenate([b[12], np.array([nt], np.int32)])
    roots = b[13][1:1 + int(b[13][0])]
    b[13] = np.concatenate([[n], roots, [nn]]).astype(np.int32)
    return b


def hand():
    """test_scene_layout's two triangles under an inner root, with the row ids a refit plan asks for"""
    b = dict(hand_scene()[0])
    b[11] = b[11].copy(); b[11][0::3] = np.arange(b[11].size // 3)
    return b


def empty_leaf():
    """the second leaf's range is (1, 1): it keeps its box through every refit"""
    return edit((hand(), None), 10, 16 + 7, 1.0)[0]


def unordered_80():
    """a foreign binding 10 whose first child box has min.x > max.x"""
    return edit((hand(), None), 10, 8, 5.0)[0]


def scenes(pt):
    """{name: complete buffers}"""
    if "scenes" not in _CACHE:
        out = {}
        for name, b in RC.extra(pt).items():
            out[name] = complete(pt, b)
        # (the 180 heights of `ladder` and the 256 of `chain256` are more than the 64-entry traversal stack allows: layoutScene refuses both scenes,
        #  so no context ever holds them; their shorter forms are what can move)
        sc = pt.hostlib.Scene(); sc.addMaterial("m")
        sc.addObjectText(RC.ladder_text(60), 0)
        out["ladder60"] = complete(pt, sc.pack())
        out["chain60"] = complete(pt, RC.chain(60))
        out["objects70"] = complete(pt, many_objects(pt), cam=(7.0, 5.0, -16.0))
        out["leafroot"] = complete(pt, with_leaf_root(pt), cam=(7.0, 0.5, -12.0))
        out["emptyleaf"] = complete(pt, empty_leaf(), cam=(1.5, 0.5, -4.0))
        out["unordered80"] = complete(pt, unordered_80(), cam=(1.5, 0.5, -4.0))
        out["hand"] = complete(pt, hand(), cam=(1.5, 0.5, -4.0))
        _CACHE["scenes"] = out
    return _CACHE["scenes"]


def infinite_vertex(tris):
    """triangle 0 with two vertices at x = +inf: e1.x = inf - inf, a NaN, as the host's subtraction gives it; the refit allows infinities"""
    t = np.array(tris, f32)
    t[0] = np.inf; t[4] = np.inf
    return t


def move_of(b, tris):
    """(new binding 3, the binding 10 the model refits to it)"""
    data, _ = RM.refit(b[10], b[11], b[12], b[13], tris)
    return np.ascontiguousarray(tris, f32), np.ascontiguousarray(data, f32)


def moved(pt, name, seed=7):
    """the shared move of a scene of scenes(): every vertex perturbed"""
    key = ("moved", name, seed)
    if key not in _CACHE:
        b = scenes(pt)[name]
        tris = RC.perturbed(b[3], seed)
        _CACHE[key] = move_of(b, tris)
    return _CACHE[key]


def workload_inputs(wl):
    tex = {0: wl.sky}
    tex.update(wl.textures)
    return dict(wl.buffers), tex

