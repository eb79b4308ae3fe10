"""CPU: the surface of include/pt_pose.h — the exported symbols, a strict-C99 client, the Python layer, and the refusals that need no device."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

import _pose_model as PM
from test_adaptive_abi import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ["pt_pose_create", "pt_pose_destroy", "pt_pose_geometry", "pt_pose_triangles"]


@pytest.fixture(scope="module")
def lib(pt):
    from pathtracer_0_amd import build
    return ctypes.CDLL(build.build_hip())


def test_hip_library_exports_the_pose_symbols(lib):
    assert _declared("pt_pose.h") == NAMES
    assert "pt_debug_pose_time" in _declared("pt_debug.h")
    for n in NAMES + ["pt_debug_pose_time"]:
        assert hasattr(lib, n), n
    for other in sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h"))):
        if other != "pt_pose.h":
            assert not set(NAMES) & set(_declared(other)), other


def test_pose_header_compiles_as_c99(tmp_path):
    src = tmp_path / "client.c"
    src.write_text('#include "pt_pose.h"\n#include "pt_debug.h"\n#include <stddef.h>\n'
                   "int main(void) {\n"
                   "    int (*c)(pt_ctx*, const int32_t*, size_t, int, pt_pose**) = pt_pose_create;\n"
                   "    int (*g)(pt_ctx*, pt_pose*, const float*, size_t, const float*, size_t, double*, int*) = pt_pose_geometry;\n"
                   "    int (*t)(pt_pose*, const float*, size_t, float*, size_t) = pt_pose_triangles;\n"
                   "    void (*d)(pt_pose*) = pt_pose_destroy;\n"
                   "    int (*p)(pt_pose*, const float*, size_t, int, int, float*) = pt_debug_pose_time;\n"
                   "    return (c == NULL) + (g == NULL) + (t == NULL) + (d == NULL) + (p == NULL) + (PT_POSE_MAX_PARTS != 65536) + (PT_POSE_RECORD_FLOATS != 24);\n}\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "client.o")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr


def test_the_refusals_that_need_no_device(lib):
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.pt_pose_create.argtypes = [vp, vp, sz, ci, vp]
    lib.pt_pose_geometry.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp]
    lib.pt_pose_triangles.argtypes = [vp, vp, sz, vp, sz]
    lib.pt_pose_destroy.argtypes = [vp]
    lib.pt_pose_destroy.restype = None
    lib.pt_last_error.restype = ctypes.c_char_p
    part = np.zeros(4, np.int32)
    out = ctypes.c_void_p(0)
    x = np.zeros(24, f32)
    tris = np.full(40, 7.0, f32)
    cost = np.full(2, -3.0)
    flag = ctypes.c_int(-5)
    fake = ctypes.c_int(0)                                             # a context / pose that is never read: null and the registry answer first
    assert lib.pt_pose_create(None, part.ctypes.data, part.nbytes, 1, ctypes.byref(out)) == -1 and lib.pt_last_error() == b"pt_pose_create: null ctx, tri_part or out"
    assert out.value is None
    assert lib.pt_pose_geometry(None, ctypes.addressof(fake), x.ctypes.data, x.nbytes, None, 0, cost.ctypes.data, ctypes.byref(flag)) == -1
    assert lib.pt_last_error() == b"pt_pose_geometry: null ctx"
    for pose in (None, ctypes.addressof(fake)):                       # null, and an address that is no live pose
        assert lib.pt_pose_geometry(ctypes.addressof(fake), pose, x.ctypes.data, x.nbytes, None, 0, cost.ctypes.data, ctypes.byref(flag)) == -1
        assert lib.pt_last_error() == b"pt_pose_geometry: null or destroyed pose"
        assert lib.pt_pose_triangles(pose, x.ctypes.data, x.nbytes, tris.ctypes.data, tris.nbytes) == -1
        assert lib.pt_last_error() == b"pt_pose_triangles: null or destroyed pose"
        lib.pt_pose_destroy(pose)                                      # ignored
    assert flag.value == -5 and (cost == -3.0).all() and (tris == 7.0).all()


def test_the_python_layer(pt):
    from pathtracer_0_amd import renderer
    for name in ("pose_create", "pose_geometry", "pose_records"):
        assert callable(getattr(renderer.Renderer, name))
    assert callable(renderer.Pose.triangles) and renderer.Renderer.pose_records is renderer.pose_records
    M = np.array([PM.rotation((1, 2, 3), 0.4, (1, 2, 3), 1.5), PM.rotation((0, 0, 1), -1.0)])
    X = renderer.pose_records(M)
    assert X.dtype == f32 and X.shape == (2, 24) and np.array_equal(X.view(np.uint32), PM.records(M).view(np.uint32))
    M4 = np.concatenate([M, np.broadcast_to([0, 0, 0, 1.0], (2, 1, 4))], axis=1)
    assert np.array_equal(renderer.pose_records(M4), X)                # 4 x 4: the last row is dropped
    N = np.arange(18.0).reshape(2, 3, 3)
    assert np.array_equal(renderer.pose_records(M, N)[:, 12:21], N.reshape(2, 9).astype(f32))
    assert renderer.pose_records(np.zeros((0, 3, 4))).shape == (0, 24)
    assert renderer.pose_records(M[0]).shape == (1, 24)
