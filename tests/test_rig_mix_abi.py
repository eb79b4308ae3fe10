"""CPU: the surface of include/pt_rig_mix.h — the five exported symbols and the debug timer, a strict-C99 and a C++ client (the layer is 24 bytes),
the Python layer's argument types and the packing of layers, and the refusals that need no device."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

from test_adaptive_abi import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ["pt_rig_mix_clip", "pt_rig_mix_mask", "pt_rig_mix_locals", "pt_rig_mix_records", "pt_rig_mix_pose_geometry"]


@pytest.fixture(scope="module")
def lib(pt):
    from pathtracer_0_amd import build
    return ctypes.CDLL(build.build_hip())


def test_hip_library_exports_the_five_mix_symbols(lib):
    assert _declared("pt_rig_mix.h") == sorted(NAMES) and len(NAMES) == 5
    assert "pt_debug_rig_mix_time" in _declared("pt_debug.h")
    for n in NAMES + ["pt_debug_rig_mix_time"]:
        assert hasattr(lib, n), n
    for other in sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h"))):
        if other != "pt_rig_mix.h":
            assert not set(NAMES) & set(_declared(other)), other
    assert _declared("pt_rig.h") == sorted(["pt_rig_create", "pt_rig_records", "pt_rig_pose_geometry", "pt_rig_clip_attach", "pt_rig_clip_records", "pt_rig_clip_pose_geometry",
                                            "pt_rig_destroy"])        # the rig's header declares what it declared


CLIENT = ('#include "pt_debug.h"\n#include "pt_rig_mix.h"\n#include <stddef.h>\n'
          "typedef char layer_is_24_bytes[sizeof(pt_rig_layer) == 24 ? 1 : -1];\n"
          "typedef char t_lies_at_16[offsetof(pt_rig_layer, t) == 16 && offsetof(pt_rig_layer, weight) == 20 && offsetof(pt_rig_layer, mask) == 4 ? 1 : -1];\n"
          "int main(void) {\n"
          "    int (*c)(pt_rig*, int, int, const float*, size_t, const float*, size_t) = pt_rig_mix_clip;\n"
          "    int (*m)(pt_rig*, int, const float*, size_t) = pt_rig_mix_mask;\n"
          "    int (*l)(pt_rig*, const pt_rig_layer*, size_t, float*, size_t) = pt_rig_mix_locals;\n"
          "    int (*r)(pt_rig*, const pt_rig_layer*, size_t, float*, size_t) = pt_rig_mix_records;\n"
          "    int (*g)(pt_ctx*, pt_rig*, const pt_rig_layer*, size_t, const float*, size_t, double*, int*) = pt_rig_mix_pose_geometry;\n"
          "    int (*t)(struct pt_rig*, const struct pt_rig_layer*, size_t, int, float*) = pt_debug_rig_mix_time;\n"
          "    pt_rig_layer y = {3, -1, PT_RIG_MIX_ADDITIVE, PT_RIG_MIX_LOOP, 0.5f, 1.0f};\n"
          "    return (c == NULL) + (m == NULL) + (l == NULL) + (r == NULL) + (g == NULL) + (t == NULL) + (y.clip != 3) + (PT_RIG_MIX_SLOTS != 16) + (PT_RIG_MIX_MASKS != 8)\n"
          "           + (PT_RIG_MIX_MAX_LAYERS != 8) + (PT_RIG_MIX_OVERRIDE != 0) + (PT_RIG_MIX_ADDITIVE != 1) + (PT_RIG_MIX_CLAMP != 0) + (PT_RIG_MIX_LOOP != 1);\n}\n")


@pytest.mark.parametrize("cc, std, name", [("gcc", "-std=c99", "client.c"), ("g++", "-std=c++17", "client.cpp")], ids=["c99", "c++"])
def test_mix_header_compiles_as_c99_and_as_cpp_and_a_layer_is_24_bytes(tmp_path, cc, std, name):
    src = tmp_path / name
    src.write_text(CLIENT)
    exe = str(tmp_path / "client")
    out = subprocess.run([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", exe + ".o"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr


def test_the_refusals_that_need_no_device(lib):
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.pt_rig_mix_clip.argtypes = [vp, ci, ci, vp, sz, vp, sz]
    lib.pt_rig_mix_mask.argtypes = [vp, ci, vp, sz]
    lib.pt_rig_mix_locals.argtypes = [vp, vp, sz, vp, sz]
    lib.pt_rig_mix_records.argtypes = [vp, vp, sz, vp, sz]
    lib.pt_rig_mix_pose_geometry.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp]
    lib.pt_debug_rig_mix_time.argtypes = [vp, vp, sz, ci, vp]
    lib.pt_last_error.restype = ctypes.c_char_p
    fake = ctypes.c_int(0)                                             # an address that is no live rig or context: never followed
    at = ctypes.addressof(fake)
    x, loc, rec, best = np.zeros(12, f32), np.zeros(12, f32), np.zeros(24, f32), ctypes.c_float(-2.0)
    y = np.zeros(6, np.int32); y[1] = -1; y[4:] = np.array([0.5, 1.0], f32).view(np.int32)      # one good layer
    for rig in (None, at):                                             # null, and an address that is no live rig
        assert lib.pt_rig_mix_clip(rig, 0, 1, x.ctypes.data, 4, x.ctypes.data, 48) == -1 and lib.pt_last_error() == b"pt_rig_mix_clip: null or destroyed rig"
        assert lib.pt_rig_mix_clip(rig, 99, 1, x.ctypes.data, 4, x.ctypes.data, 48) == -1 and lib.pt_last_error() == b"pt_rig_mix_clip: null or destroyed rig"
        assert lib.pt_rig_mix_mask(rig, 0, x.ctypes.data, 4) == -1 and lib.pt_last_error() == b"pt_rig_mix_mask: null or destroyed rig"
        assert lib.pt_rig_mix_locals(rig, y.ctypes.data, 24, loc.ctypes.data, 48) == -1 and lib.pt_last_error() == b"pt_rig_mix_locals: null or destroyed rig"
        assert lib.pt_rig_mix_locals(rig, None, 0, None, 0) == -1 and lib.pt_last_error() == b"pt_rig_mix_locals: null or destroyed rig"
        assert lib.pt_rig_mix_records(rig, y.ctypes.data, 24, rec.ctypes.data, 96) == -1 and lib.pt_last_error() == b"pt_rig_mix_records: null or destroyed rig"
        assert lib.pt_rig_mix_pose_geometry(None, rig, y.ctypes.data, 24, None, 0, None, None) == -1 and lib.pt_last_error() == b"pt_rig_mix_pose_geometry: null ctx"
        assert lib.pt_rig_mix_pose_geometry(at, rig, y.ctypes.data, 24, None, 0, None, None) == -1 and lib.pt_last_error() == b"pt_rig_mix_pose_geometry: null or destroyed rig"
        assert lib.pt_debug_rig_mix_time(rig, y.ctypes.data, 24, 1, ctypes.addressof(best)) == -1 and lib.pt_last_error() == b"pt_debug_rig_mix_time: bad argument"
    assert best.value == -2.0 and not rec.any() and not loc.any()


def test_the_python_layer_declares_the_mix_calls(pt):
    from pathtracer_0_amd import renderer
    import inspect
    L = renderer.lib()
    want = dict(pt_rig_mix_clip=7, pt_rig_mix_mask=4, pt_rig_mix_locals=5, pt_rig_mix_records=5, pt_rig_mix_pose_geometry=8, pt_debug_rig_mix_time=5)
    for name, n in want.items():
        assert len(getattr(L, name).argtypes) == n, name
    for name, params in dict(mix_clip=["slot", "times", "values"], mask=["slot", "weights"], mix_locals=["layers"], mix_records=["layers"], mix=["layers", "ellip"]).items():
        assert list(inspect.signature(getattr(renderer.Rig, name)).parameters)[1:] == params, name
    assert renderer.RIG_LAYER.itemsize == 24 and renderer.RIG_LAYER.names == ("clip", "mask", "mode", "wrap", "t", "weight")
    y = renderer.rig_layers([(2, 0.5), dict(clip=3, t=1.5, weight=0.25, mask=7, mode="additive", wrap="loop"), (4, -1.0, 0.5, 1, 1, 0)])
    assert y.dtype == renderer.RIG_LAYER and y.tolist() == [(2, -1, 0, 0, 0.5, 1.0), (3, 7, 1, 1, 1.5, 0.25), (4, 1, 1, 0, -1.0, 0.5)]
    assert renderer.rig_layers(y) is not None and np.array_equal(renderer.rig_layers(y), y) and renderer.rig_layers([]).nbytes == 0
    with pytest.raises(ValueError):
        renderer.rig_layers([dict(clip=1)])
    with pytest.raises(ValueError):
        renderer.rig_layers([dict(clip=1, t=0.0, speed=2.0)])
