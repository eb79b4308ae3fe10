"""CPU: the host-only layout step of the scene build (csrc/hip/pt_scene_layout.hpp) through tests/c/scene_layout_check.cpp, a stand-alone program
built twice with g++: plain, and under the address / undefined-behaviour / float-cast sanitizers (which must stay silent on every case).

  * the arrays, counts and modes it builds for the workloads of scenes.py equal, digest for digest, what buildScene built before the split
    (tests/golden/scene_layout_parent.json, recorded from that commit's buildScene);
  * every refusal of the function: code -4 and the exact text;
  * accepted edge cases and the mode each one decides."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_layout_parent.json")
OPTION_NAMES = ("bfsNodes", "asmNodeLayout", "asmNoRootCull", "forceNiBits8", "ldsBudget", "extendCacheBytes", "stackModeForce", "asmNodes80Limit")
DEFAULTS = dict(bfsNodes=0x7fffffff, asmNodeLayout=-1, asmNoRootCull=0, forceNiBits8=0, ldsBudget=20 * 1024, extendCacheBytes=8 * 1024, stackModeForce=-1,
                asmNodes80Limit=2 << 20)
NAN = float("nan")


# ------------------------------------------------------------------------------------------ the program and its input file
def _build(tmp, name, extra):
    exe = str(tmp / name)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include")] + extra + \
          ["-o", exe, os.path.join(ROOT, "tests", "c", "scene_layout_check.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr      # no warning either
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scene_layout")
    return tmp, [_build(tmp, "check_plain", []),
                 _build(tmp, "check_san", ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"])]


def write_scene(path, buffers, textures, **options):
    """buffers: {binding: array of float32 / int32}; textures: {index: (h, w, 4) uint8}, index 0 the sky"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(buffers)))
        for b, arr in buffers.items():
            arr = np.ascontiguousarray(arr)
            assert arr.dtype in (np.float32, np.int32), (b, arr.dtype)
            f.write(struct.pack("<iQ", b, arr.size)); f.write(arr.tobytes())
        f.write(struct.pack("<I", len(textures)))
        for idx, t in textures.items():
            t = np.ascontiguousarray(t, dtype=np.uint8)
            f.write(struct.pack("<iii", idx, t.shape[1], t.shape[0])); f.write(t.tobytes())
        opts = dict(DEFAULTS); opts.update(options)
        f.write(struct.pack("<8i", *(opts[k] for k in OPTION_NAMES)))


def parse(stdout):
    out = {}
    for line in stdout.splitlines():
        k, _, v = line.partition(" ")
        out[k] = v
    return out


def run_all(programs, name, buffers, textures, **options):
    """the case through both builds of the program: the same output, nothing on stderr, exit 0"""
    tmp, exes = programs
    path = str(tmp / (name + ".scene"))
    write_scene(path, buffers, textures, **options)
    outs = []
    for exe in exes:
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stderr == "", (exe, name, r.returncode, r.stderr[-2000:])
        outs.append(r.stdout)
    os.remove(path)
    assert outs[0] == outs[1], name
    return parse(outs[0])


# ------------------------------------------------------------------------------------------ same bytes as before the split
_workloads = {}


def workload(pt, name):
    if name not in _workloads:
        _workloads[name] = pt.scenes.build(name, 48, 48 if name == "C1" else 27)      # (the layout reads no image size)
    return _workloads[name]


def workload_inputs(wl):
    tex = {0: wl.sky}
    tex.update(wl.textures)
    return dict(wl.buffers), tex


VARIANTS = [("bfs7", dict(bfsNodes=7)), ("layout0", dict(asmNodeLayout=0)), ("layout1", dict(asmNodeLayout=1)), ("ni8", dict(forceNiBits8=1)),
            ("ni32", dict(forceNiBits8=2)), ("stack1", dict(stackModeForce=1)), ("stack2", dict(stackModeForce=2)), ("lds0", dict(ldsBudget=0)),
            ("cache64k", dict(extendCacheBytes=64 * 1024))]
GOLDEN_CASES = [(s, "default", {}) for s in ("C1", "C2", "C3", "C4", "C5", "C6", "T1", "M1")] + \
               [(s, v, o) for s in ("T1", "C3", "C6") for v, o in VARIANTS] + [("C6", "nocull", dict(asmNoRootCull=1))]


@pytest.mark.parametrize("scene,variant,options", GOLDEN_CASES, ids=[f"{s}-{v}" for s, v, _ in GOLDEN_CASES])
def test_layout_equals_what_buildscene_built_before_the_split(pt, programs, scene, variant, options):
    want = json.load(open(GOLDEN))[f"{scene}-{variant}"]
    buffers, tex = workload_inputs(workload(pt, scene))
    got = run_all(programs, f"{scene}-{variant}", buffers, tex, **options)
    assert got == want
    if scene == "C4":                                            # the one workload beyond 26 214 inner nodes: the automatic stride is 64
        assert int(got["nInner"]) > 26214 and got["asmNodeStride"] == "64"


# ------------------------------------------------------------------------------------------ hand-made scenes
def material(**F):
    """one 48-float record; keywords F<k>=value set mtlData[48 m + k] (the k of the layout step's F[k]); no maps"""
    r = np.zeros(48, np.float32)
    for k in (22, 23, 24, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41):
        r[k - 1] = -1.0
    r[3:6] = 0.8; r[25] = 1.0                                    # Kd, Pr
    for k, v in F.items():
        r[int(k[1:]) - 1] = v
    return r


def materials(*recs):
    return np.concatenate([np.array([48.0], np.float32)] + list(recs)).astype(np.float32)


def triangle(mat=0.0, dx=0.0):
    t = np.zeros(40, np.float32)
    t[0:3] = (dx, 0, 0); t[4:7] = (dx + 1, 0, 0); t[8:11] = (dx, 1, 0); t[36] = mat
    return t


def box(lo, hi, s=0.0, e=0.0):
    return np.array(list(lo) + list(hi) + [s, e], np.float32)


def hand_scene():
    """two triangles, three nodes (an inner root over two leaves), one object, one material, no ellipsoid"""
    b = {0: np.array([0, 0, -3], np.float32), 1: np.zeros(3, np.float32), 2: np.array([-1e6, -1e6, 0], np.float32),
         3: np.concatenate([triangle(), triangle(dx=2.0)]),
         4: np.array([1.5, 1.0, 48, 27 / 48, 8, 8, 2.2, 0.001, 1.0, 1.0, 0.0, 1.0], np.float32),
         5: np.array([0.0], np.float32), 7: np.array([0.0], np.float32),
         10: np.concatenate([box((0, 0, 0), (3, 1, 0)), box((0, 0, 0), (1, 1, 0), 0, 1), box((2, 0, 0), (3, 1, 0), 1, 2)]),
         11: np.array([0, 1, 2, 0, -1, -1, 0, -1, -1], np.int32), 12: np.array([0, 1], np.int32), 13: np.array([1, 0], np.int32),
         14: materials(material())}
    return b, {0: np.full((1, 1, 4), 200, np.uint8)}


def leaf_roots(n, shared_triangle=False):
    """n objects, each a leaf root over one triangle of its own (or all over triangle 0)"""
    b, tex = hand_scene()
    b[3] = np.concatenate([triangle(dx=2.0 * k) for k in range(n)])
    b[10] = np.concatenate([box((2 * k, 0, 0), (2 * k + 1, 1, 0), k, k + 1) for k in range(n)])
    b[11] = np.array([0, -1, -1] * n, np.int32)
    b[12] = np.zeros(n, np.int32) if shared_triangle else np.arange(n, dtype=np.int32)
    b[13] = np.array([n] + list(range(n)), np.int32)
    return b, tex


def chain(levels):
    """one object whose tree is a left-leaning chain of `levels` inner nodes over empty leaves"""
    b, tex = hand_scene()
    tree, n = [], 2 * levels + 1
    for k in range(levels):                                      # inner node k: left = the next inner node (the last one: a leaf), right = a leaf
        tree += [0, k + 1 if k + 1 < levels else 2 * levels, levels + k]
    tree += [0, -1, -1] * (levels + 1)
    b[11] = np.array(tree, np.int32)
    b[10] = np.concatenate([box((0, 0, 0), (1, 1, 1))] * n)
    return b, tex


def edit(scene, binding, index, value):
    b, tex = scene
    b = dict(b); a = b[binding].copy(); a[index] = value; b[binding] = a
    return b, tex


def replace(scene, binding, array):
    b, tex = scene
    b = dict(b); b[binding] = array
    return b, tex


E_PARAMS = "Parameters buffer (binding 4) must hold 12 floats"
E_CAMERA = "ORIGIN/ROTATION (bindings 0,1) not set"
E_MOUSE = "MOUSE_POS (binding 2) not set"
E_MTL = "mtlData (binding 14) not set"
E_OBJ = "objIndices (binding 13) not set"
E_IMP = "ImpData (binding 5) not set: [count, fn x n, shift x 3n, scale x 3n, rot x 3n, mat x n]; send [0] for none"
E_ELLIP = "EllipData (binding 7) not set"
E_SKY = "texture 0 (sky) not set"
E_BVHDATA = "BVHdata shorter than 8 floats per BVHtree node"
E_MTL0 = "mtlData[0] (floats per material) must be >= 48"
E_TEX = "a material names a texture index that was never uploaded with pt_set_texture"
E_OBJ0 = "objIndices[0] exceeds the buffer"
E_ROOT = "objIndices root out of range"
E_TWICE = "BVH node reachable twice (not a tree)"
E_CHILD = "BVHtree child index out of range"
E_DEEP = "BVH too deep for the reference's `int stack[64]` (frag.glsl:465)"
E_LEAF = "leaf index range outside leafTriIndices"
E_LEAFTRI = "leafTriIndices entry outside the triangle buffer"
E_TRIMAT = "triangle material index out of range (SURVEY.md Q-14: OBJ faces before any o/g line get -1)"
E_ELLIPLEN = "EllipData shorter than its count says"
E_ELLIPMAT = "ellipsoid material index out of range"


def five_nodes(tree):
    """an inner root over two inner nodes that both name the leaves 3 and 4"""
    b, tex = hand_scene()
    b[11] = np.array(tree, np.int32)
    b[10] = np.concatenate([box((0, 0, 0), (3, 1, 0))] * 3 + [box((0, 0, 0), (1, 1, 0), 0, 1), box((2, 0, 0), (3, 1, 0), 1, 2)])
    return b, tex


def one_ellipsoid(mat):
    return np.array([1.0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0.5, mat], np.float32)


def refusals():
    H = hand_scene()
    no_sky = (H[0], {})
    tex3 = (replace(H, 14, materials(material(F23=2.0)))[0], {0: H[1][0], 3: np.zeros((2, 2, 4), np.uint8)})
    return [
        ("params_short", replace(H, 4, H[0][4][:11]), E_PARAMS),
        ("no_origin", replace(H, 0, np.zeros(0, np.float32)), E_CAMERA),
        ("no_rotation", replace(H, 1, np.zeros(0, np.float32)), E_CAMERA),
        ("no_mouse", replace(H, 2, np.zeros(0, np.float32)), E_MOUSE),
        ("no_materials", replace(H, 14, np.zeros(0, np.float32)), E_MTL),
        ("no_objindices", replace(H, 13, np.zeros(0, np.int32)), E_OBJ),
        ("no_impdata", replace(H, 5, np.zeros(0, np.float32)), E_IMP),
        ("impdata_negative", edit(H, 5, 0, -1.0), E_IMP),
        ("impdata_nan", edit(H, 5, 0, NAN), E_IMP),
        ("no_ellipdata", replace(H, 7, np.zeros(0, np.float32)), E_ELLIP),
        ("no_sky", no_sky, E_SKY),
        ("bvhdata_short", replace(H, 10, H[0][10][:23]), E_BVHDATA),
        ("mtl0_47", edit(H, 14, 0, 47.0), E_MTL0),
        ("mtl0_nan", edit(H, 14, 0, NAN), E_MTL0),
        ("texture_beyond_table", replace(H, 14, materials(material(F23=5.0))), E_TEX),
        ("texture_never_uploaded", tex3, E_TEX),
        ("objcount_beyond_buffer", edit(H, 13, 0, 5), E_OBJ0),
        ("objcount_negative", edit(H, 13, 0, -1), E_OBJ0),
        ("root_too_large", edit(H, 13, 1, 3), E_ROOT),
        ("root_negative", edit(H, 13, 1, -1), E_ROOT),
        ("two_objects_one_root", replace(H, 13, np.array([2, 0, 0], np.int32)), E_TWICE),
        ("child_negative", replace(H, 11, np.array([0, -2, -2, 0, -1, -1, 0, -1, -1], np.int32)), E_CHILD),
        ("child_too_large", edit(H, 11, 2, 3), E_CHILD),
        ("child_is_its_ancestor", replace(H, 11, np.array([0, 1, 2, 0, 0, 2, 0, -1, -1], np.int32)), E_TWICE),
        ("two_parents_one_child", five_nodes([0, 1, 2, 0, 3, 4, 0, 3, 4, 0, -1, -1, 0, -1, -1]), E_TWICE),
        ("chain_64_inner_levels", chain(64), E_DEEP),
        ("leaf_start_negative", edit(H, 10, 8 + 6, -1.0), E_LEAF),
        ("leaf_end_too_large", edit(H, 10, 16 + 7, 3.0), E_LEAF),
        ("leaf_start_nan", edit(H, 10, 8 + 6, NAN), E_LEAF),
        ("leaftri_too_large", edit(H, 12, 0, 2), E_LEAFTRI),
        ("leaftri_negative", edit(H, 12, 1, -1), E_LEAFTRI),
        ("trimat_minus_one", edit(H, 3, 36, -1.0), E_TRIMAT),
        ("trimat_nmat", edit(H, 3, 40 + 36, 1.0), E_TRIMAT),
        ("trimat_nan", edit(H, 3, 36, NAN), E_TRIMAT),
        ("ellipdata_short", replace(H, 7, one_ellipsoid(0.0)[:11]), E_ELLIPLEN),
        ("ellipcount_1e30", edit(H, 7, 0, 1e30), E_ELLIPLEN),
        ("ellipcount_nan", edit(H, 7, 0, NAN), E_ELLIPLEN),
        ("ellipmat_too_large", replace(H, 7, one_ellipsoid(5.0)), E_ELLIPMAT),
        ("ellipmat_negative", replace(H, 7, one_ellipsoid(-1.0)), E_ELLIPMAT),
        ("ellipmat_nan", replace(H, 7, one_ellipsoid(NAN)), E_ELLIPMAT),
    ]


REFUSALS = refusals()


@pytest.mark.parametrize("name,scene,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(programs, name, scene, text):
    got = run_all(programs, name, *scene)
    assert got == {"rc": "-4", "err": text}


def test_refusals_of_the_textured_workload(pt, programs):
    """the same exits from a real workload's buffers (T1: textures, several materials)"""
    b, tex = workload_inputs(workload(pt, "T1"))
    assert run_all(programs, "T1-ok", b, tex)["rc"] == "0"
    cases = [(edit((b, tex), 11, 1, len(b[11]) // 3), E_CHILD), (edit((b, tex), 11, 1, 0), E_TWICE), (edit((b, tex), 3, 36, 1000.0), E_TRIMAT),
             (replace((b, tex), 7, one_ellipsoid(0.0)[:11]), E_ELLIPLEN), ((b, {0: tex[0]}), E_TEX)]
    assert len(tex) > 1
    for k, (scene, text) in enumerate(cases):
        assert run_all(programs, f"T1-refused{k}", *scene) == {"rc": "-4", "err": text}, k


def nine_refraction_indices(transmissive):
    recs = [material(F16=1.1 + 0.05 * k, F12=(0.5 if transmissive and k == 0 else 0.0)) for k in range(9)]
    return replace(hand_scene(), 14, materials(*recs))


ACCEPTED = [
    ("empty_leaf", edit(hand_scene(), 10, 16 + 7, 1.0), {}, dict(asmEligible="0", asmWhyNot="a leaf without triangles", nTriRecs="1")),
    ("leaf_root", edit(hand_scene(), 13, 1, 1), {}, dict(nInner="0", nTriRecs="1", numObj="1", stackDepth="1", asmEligible="1", asmWhyNot="")),
    ("inverted_box_80", edit(hand_scene(), 10, 8, 5.0), dict(asmNodeLayout=0), dict(asmNodeStride="80", asmEligible="0", asmWhyNot="a node box with min > max or a NaN")),
    ("inverted_box_auto", edit(hand_scene(), 10, 8, 5.0), {}, dict(asmNodeStride="80", asmEligible="0", asmWhyNot="a node box with min > max or a NaN")),
    ("inverted_box_64", edit(hand_scene(), 10, 8, 5.0), dict(asmNodeLayout=1), dict(asmNodeStride="64", asmEligible="1", asmWhyNot="")),
    ("objects_8", leaf_roots(8), {}, dict(numObj="8", asmGroupShift="0", roots_bytes=8 * 32)),
    ("objects_9", leaf_roots(9), {}, dict(numObj="9", asmGroupShift="0", roots_bytes=(9 + 64) * 32)),
    ("objects_65", leaf_roots(65), {}, dict(numObj="65", asmGroupShift="1", roots_bytes=(65 + 64) * 32)),
    ("shared_triangle", leaf_roots(2, shared_triangle=True), {}, dict(ambiguousTriObj="1")),
    ("own_triangles", leaf_roots(2), {}, dict(ambiguousTriObj="0")),
    ("nine_ni_transmissive", nine_refraction_indices(True), {}, dict(trans="1", niBits="8", numMat="9")),
    ("nine_ni_opaque", nine_refraction_indices(False), {}, dict(trans="0", niBits="0", numMat="9")),
    ("one_ni_transmissive", replace(hand_scene(), 14, materials(material(F12=0.5, F16=1.5))), {}, dict(trans="1", niBits="3")),
    ("chain_63_inner_levels", chain(63), {}, dict(stackDepth="64", nInner="63", asmEligible="0", asmWhyNot="a leaf without triangles")),
    ("leaf_end_nan_is_an_empty_leaf", edit(hand_scene(), 10, 16 + 7, NAN), {}, dict(nTriRecs="1", asmWhyNot="a leaf without triangles")),
]


@pytest.mark.parametrize("name,scene,options,want", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_accepted_edge_case(programs, name, scene, options, want):
    got = run_all(programs, name, *scene, **options)
    assert got["rc"] == "0" and got["err"] == ""
    want = dict(want)
    if "roots_bytes" in want:
        assert int(got["roots"].split()[1]) == want.pop("roots_bytes")
    assert {k: got[k] for k in want} == want

