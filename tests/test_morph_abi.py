"""CPU: the surface of include/pt_morph.h — the exported symbols, a strict-C99 and a C++ client, the Python layer, and the refusals that need no
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
NAMES = ["pt_morph_attach", "pt_morph_weights"]


@pytest.fixture(scope="module")
def lib(pt):
    from pathtracer_0_amd import build
    return ctypes.CDLL(build.build_hip())


def test_hip_library_exports_the_morph_symbols(lib):
    assert _declared("pt_morph.h") == NAMES
    assert {"pt_debug_morph_time", "pt_debug_morph_rest"} <= set(_declared("pt_debug.h"))
    for n in NAMES + _declared("pt_debug.h") + _declared("pt_pose.h") + _declared("pt_skin.h"):
        assert hasattr(lib, n), n
    for other in sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h"))):
        if other != "pt_morph.h":
            assert not set(NAMES) & set(_declared(other)), other


def test_the_unit_is_built_and_the_kernel_hash_is_the_parent_s(pt):
    from pathtracer_0_amd import build
    assert "pt_morph.hip" in build.HIP_UNITS and os.path.exists(os.path.join(ROOT, "pathtracer-0_amd", "csrc", "hip", "pt_morph.hip"))
    assert not any("morph" in f for f in build.KERNEL_HASH_FILES)        # a scene-build file: kernel_source_hash() does not cover it


CLIENT = ('#include "pt_morph.h"\n#include "pt_debug.h"\n#include <stddef.h>\n'
          "int main(void) {\n"
          "    int (*a)(pt_pose*, int, const int64_t*, size_t, const int32_t*, size_t, const float*, size_t) = pt_morph_attach;\n"
          "    int (*w)(pt_pose*, const float*, size_t) = pt_morph_weights;\n"
          "    int (*t)(struct pt_pose*, const float*, size_t, int, float*) = pt_debug_morph_time;\n"
          "    int (*r)(struct pt_pose*, float*, size_t) = pt_debug_morph_rest;\n"
          "    return (a == NULL) + (w == NULL) + (t == NULL) + (r == NULL) + (PT_MORPH_MAX_TARGETS != 1024) + (PT_POSE_MAX_PARTS != 65536);\n}\n")


@pytest.mark.parametrize("cc, std, name", [("gcc", "-std=c99", "client.c"), ("g++", "-std=c++17", "client.cpp")], ids=["c99", "c++"])
def test_morph_header_compiles_as_c99_and_as_cpp(tmp_path, cc, std, name):
    src = tmp_path / name
    src.write_text(CLIENT)
    out = subprocess.run([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "client.o")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr


def test_the_refusals_that_need_no_device(lib):
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.pt_morph_attach.argtypes = [vp, ci, vp, sz, vp, sz, vp, sz]
    lib.pt_morph_weights.argtypes = [vp, vp, sz]
    lib.pt_debug_morph_time.argtypes = [vp, vp, sz, ci, vp]
    lib.pt_debug_morph_rest.argtypes = [vp, vp, sz]
    lib.pt_last_error.restype = ctypes.c_char_p
    start = np.array([0, 1], np.int64)
    corner = np.zeros(1, np.int32)
    delta = np.zeros(6, f32)
    w = np.zeros(1, f32)
    fake = ctypes.c_int(0)                                             # an address that is no live pose: never followed
    best = ctypes.c_float(-2.0)
    out = np.zeros(40, f32)
    for pose in (None, ctypes.addressof(fake)):
        assert lib.pt_morph_attach(pose, 1, start.ctypes.data, start.nbytes, corner.ctypes.data, corner.nbytes, delta.ctypes.data, delta.nbytes) == -1
        assert lib.pt_last_error() == b"pt_morph_attach: null or destroyed pose, or null target_start, entry_corner or entry_delta"
        assert lib.pt_morph_attach(pose, 0, None, 0, None, 0, None, 0) == -1      # the first check answers whatever else is wrong
        assert lib.pt_last_error() == b"pt_morph_attach: null or destroyed pose, or null target_start, entry_corner or entry_delta"
        assert lib.pt_morph_weights(pose, w.ctypes.data, w.nbytes) == -1
        assert lib.pt_last_error() == b"pt_morph_weights: null or destroyed pose"
        assert lib.pt_morph_weights(pose, None, 0) == -1
        assert lib.pt_last_error() == b"pt_morph_weights: null or destroyed pose"
        assert lib.pt_debug_morph_time(pose, w.ctypes.data, w.nbytes, 1, ctypes.addressof(best)) == -1
        assert lib.pt_last_error() == b"pt_debug_morph_time: bad argument"
        assert lib.pt_debug_morph_rest(pose, out.ctypes.data, out.nbytes) == -1
        assert lib.pt_last_error() == b"pt_debug_morph_rest: bad argument"
    assert best.value == -2.0 and not out.any()


def test_the_python_layer(pt):
    from pathtracer_0_amd import renderer
    assert callable(renderer.Pose.morph_attach) and callable(renderer.Pose.morph_weights)
    L = renderer.lib()
    assert L.pt_morph_attach.argtypes is not None and len(L.pt_morph_attach.argtypes) == 8 and len(L.pt_debug_morph_time.argtypes) == 5
    wl, bone, weight, targets, X, w = pt.scenes.m4_bulging(3)
    n = wl.buffers[3].size // 40
    assert wl.name == "M4" and len(targets) == 3 and X.shape == (5, 24) and w.dtype == f32 and w.shape == (3,) and (w > 0).all()
    first, n_side, n_cap = wl.info["tube"]
    for c, d in targets:
        assert c.dtype == np.int32 and d.dtype == f32 and d.shape == (c.size, 6) and c.size > 100 and np.unique(c).size == c.size
        assert c.min() >= 3 * first and c.max() < 3 * (first + n_side) and np.isfinite(d).all()
        assert (bone.reshape(-1, 4)[c, 0] >= 0).all()                  # only corners the skin moves
        tris = wl.buffers[3].reshape(-1, 40)
        k, cc = c // 3, c % 3
        nrm = np.stack([tris[k, 12 + 4 * cc + j] for j in range(3)], axis=1)
        along = (d[:, :3] * nrm).sum(axis=1) / np.linalg.norm(nrm, axis=1)
        assert np.allclose(along, np.linalg.norm(d[:, :3], axis=1), rtol=1e-4, atol=1e-7)      # the vertex deltas run along the rest normal
    rest = pt.scenes.m4_bulging(0)
    m3 = pt.scenes.m3_bending(3)
    assert np.array_equal(rest[0].buffers[3].view(np.uint32), wl.buffers[3].view(np.uint32)) and not rest[5].any()      # step 0: every weight 0
    assert np.array_equal(m3[0].buffers[3].view(np.uint32), wl.buffers[3].view(np.uint32))                               # M3's tube ...
    assert np.array_equal(m3[1], bone) and np.array_equal(m3[2], weight) and np.array_equal(m3[3], X)                    # ... and skin
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(rest[3], targets))              # the targets do not depend on the step
    assert pt.scenes.build("M4").buffers[3].size == wl.buffers[3].size and n == first + n_side + n_cap
