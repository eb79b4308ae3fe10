"""CPU: the surface of include/pt_normals.h — the exported symbols, a strict-C99 and a C++ client, the Python layer, and the refusals that need no
device."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

from test_adaptive_abi import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ["pt_normals_attach", "pt_normals_mode"]


@pytest.fixture(scope="module")
def lib(pt):
    from pathtracer_0_amd import build
    return ctypes.CDLL(build.build_hip())


def test_hip_library_exports_the_normals_symbols(lib):
    assert os.path.exists(os.path.join(ROOT, "include", "pt_normals.h"))
    assert _declared("pt_normals.h") == NAMES
    assert "pt_debug_normals_time" in _declared("pt_debug.h")
    for n in NAMES + _declared("pt_debug.h") + _declared("pt_pose.h") + _declared("pt_skin.h") + _declared("pt_morph.h"):
        assert hasattr(lib, n), n
    for other in sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h"))):
        if other != "pt_normals.h":
            assert not set(NAMES) & set(_declared(other)), other
        if other != "pt_debug.h":
            assert "pt_debug_normals_time" not in _declared(other), other


def test_the_unit_is_built_and_the_kernel_hash_is_the_parent_s(pt):
    from pathtracer_0_amd import build
    d = os.path.join(ROOT, "pathtracer-0_amd", "csrc", "hip")
    assert "pt_normals.hip" in build.HIP_UNITS and os.path.exists(os.path.join(d, "pt_normals.hip"))
    assert os.path.exists(os.path.join(d, "pt_normals_launch.hpp")) and os.path.exists(os.path.join(d, "pt_normals_rule.hpp"))
    assert not any("normals" in f for f in build.KERNEL_HASH_FILES)      # a scene-build file: kernel_source_hash() does not cover it


CLIENT = ('#include "pt_normals.h"\n#include "pt_debug.h"\n#include <stddef.h>\n'
          "int main(void) {\n"
          "    int (*a)(pt_pose*, const int32_t*, size_t, int64_t, uint32_t) = pt_normals_attach;\n"
          "    int (*m)(pt_pose*, int) = pt_normals_mode;\n"
          "    int (*t)(struct pt_pose*, const float*, size_t, int, int, float*) = pt_debug_normals_time;\n"
          "    return (a == NULL) + (m == NULL) + (t == NULL) + (PT_NORMALS_FLIP != 1u) + (PT_POSE_MAX_PARTS != 65536);\n}\n")


@pytest.mark.parametrize("cc, std, name", [("gcc", "-std=c99", "client.c"), ("g++", "-std=c++17", "client.cpp")], ids=["c99", "c++"])
def test_normals_header_compiles_as_c99_and_as_cpp(tmp_path, cc, std, name):
    src = tmp_path / name
    src.write_text(CLIENT)
    out = subprocess.run([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "client.o")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr


def test_the_refusals_that_need_no_device(lib):
    assert hasattr(lib, "pt_normals_attach") and hasattr(lib, "pt_normals_mode") and hasattr(lib, "pt_debug_normals_time")
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.pt_normals_attach.argtypes = [vp, vp, sz, ctypes.c_int64, ctypes.c_uint32]
    lib.pt_normals_mode.argtypes = [vp, ci]
    lib.pt_debug_normals_time.argtypes = [vp, vp, sz, ci, ci, vp]
    lib.pt_last_error.restype = ctypes.c_char_p
    ids = np.array([0, 1, 2], np.int32)
    x = np.zeros(24, f32)
    fake = ctypes.c_int(0)                                             # an address that is no live pose: never followed
    best = ctypes.c_float(-2.0)
    for pose in (None, ctypes.addressof(fake)):
        assert lib.pt_normals_attach(pose, ids.ctypes.data, ids.nbytes, 3, 0) == -1
        assert lib.pt_last_error() == b"pt_normals_attach: null or destroyed pose, or null corner_vertex"
        assert lib.pt_normals_attach(pose, None, 0, -1, 6) == -1       # the first check answers whatever else is wrong
        assert lib.pt_last_error() == b"pt_normals_attach: null or destroyed pose, or null corner_vertex"
        for on in (0, 1, 2):
            assert lib.pt_normals_mode(pose, on) == -1
            assert lib.pt_last_error() == b"pt_normals_mode: null or destroyed pose"
        assert lib.pt_debug_normals_time(pose, x.ctypes.data, x.nbytes, 0, 1, ctypes.addressof(best)) == -1
        assert lib.pt_last_error() == b"pt_debug_normals_time: bad argument"
    assert best.value == -2.0


def test_the_python_layer(pt):
    from pathtracer_0_amd import renderer
    assert callable(renderer.Pose.normals_attach) and callable(renderer.Pose.normals_mode)
    L = renderer.lib()
    assert L.pt_normals_attach.argtypes is not None and len(L.pt_normals_attach.argtypes) == 5 and len(L.pt_debug_normals_time.argtypes) == 6
    m5 = pt.scenes.m5_rippling(3)
    m4 = pt.scenes.m4_bulging(3)
    wl, bone, weight, targets, X, w, ids, n_vertices = m5
    assert wl.name == "M5" and len(m5) == 8 and ids.dtype == np.int32 and ids.size == wl.buffers[3].size // 40 * 3
    assert np.array_equal(m4[0].buffers[3].view(np.uint32), wl.buffers[3].view(np.uint32))                                  # M4's tube ...
    assert np.array_equal(m4[1], bone) and np.array_equal(m4[2], weight) and np.array_equal(m4[4], X) and np.array_equal(m4[5], w)      # ... skin, records, weights
    first, n_side, n_cap = wl.info["tube"]
    named = np.nonzero(ids >= 0)[0]
    assert named.min() == 3 * first and named.max() == 3 * (first + n_side) - 1 and named.size == 3 * n_side      # the whole side, nothing else
    assert (bone.reshape(-1, 4)[named, 0] >= 0).all()                  # only corners the skin moves
    assert n_vertices == ids.max() + 1 == np.unique(ids[named]).size == 13 * 10      # (n_seg + 1) rings of n_around vertices: welded
    t = ids.reshape(-1, 3)
    assert all((t[:, a] != t[:, b])[t[:, a] >= 0].all() for a, b in ((0, 1), (0, 2), (1, 2)))      # once per triangle
    assert pt.scenes.build("M5").buffers[3].size == wl.buffers[3].size
    # weld_corners: by position, and with keep_creases by the rest normal too
    tris = np.zeros((2, 40), f32)
    tris[0, 0:3], tris[0, 4:7], tris[0, 8:11] = (0, 0, 0), (1, 0, 0), (0, 1, 0)
    tris[1, 0:3], tris[1, 4:7], tris[1, 8:11] = (1, 0, 0), (1, 1, 0), (0, 1, 0)
    tris[:, 14] = tris[:, 18] = tris[:, 22] = 1.0
    tris[1, 20:23] = (0.0, 1.0, 0.0)                                   # the shared vertex (0, 1, 0) with another normal in the second triangle: a crease
    both, n_both = pt.scenes.weld_corners(tris, np.arange(6), keep_creases=False)
    assert n_both == 4 and both[1] == both[3] and both[2] == both[5] and len(set(both.tolist())) == 4
    hard, n_hard = pt.scenes.weld_corners(tris, np.arange(6), keep_creases=True)
    assert n_hard == 5 and hard[1] == hard[3] and hard[2] != hard[5]
    some, n_some = pt.scenes.weld_corners(tris, np.array([0, 1, 2]))
    assert n_some == 3 and (some[3:] == -1).all() and sorted(some[:3].tolist()) == [0, 1, 2]
    none, n_none = pt.scenes.weld_corners(tris, np.zeros(0, np.int64))
    assert n_none == 0 and (none == -1).all()
    tris[0, 4:7] = tris[0, 0:3]                                        # a degenerate triangle: its second corner gets no id
    deg, n_deg = pt.scenes.weld_corners(tris, np.arange(6), keep_creases=False)
    assert deg[1] == -1 and deg[0] >= 0 and n_deg == deg.max() + 1 == np.unique(deg[deg >= 0]).size
