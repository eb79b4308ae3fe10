"""CPU: the surface of include/pt_rig_ik.h — the three exported symbols and the debug timer, a strict-C99 and a C++ client (constraint and goal
are 32 bytes each), the Python layer's argument types and packers, the workload M9, and the refusals that need no device."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

import _rig_ik_model as IM
from test_adaptive_abi import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ["pt_rig_ik_attach", "pt_rig_ik_goals", "pt_rig_ik_locals"]


@pytest.fixture(scope="module")
def lib(pt):
    from pathtracer_0_amd import build
    return ctypes.CDLL(build.build_hip())


def test_hip_library_exports_the_three_ik_symbols(lib):
    assert _declared("pt_rig_ik.h") == sorted(NAMES) and len(NAMES) == 3
    assert "pt_debug_rig_ik_time" in _declared("pt_debug.h")
    for n in NAMES + ["pt_debug_rig_ik_time"]:
        assert hasattr(lib, n), n
    for other in sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h"))):
        if other != "pt_rig_ik.h":
            assert not set(NAMES) & set(_declared(other)), other


def test_the_unit_is_built_and_the_kernel_hash_does_not_cover_it(pt):
    from pathtracer_0_amd import build
    assert "pt_rig_ik.hip" in build.HIP_UNITS and not any("rig" in f for f in build.KERNEL_HASH_FILES)
    for f in ("pt_rig_ik.hip", "pt_rig_ik_launch.hpp", "pt_rig_ik_rule.hpp", "pt_rig_ik_steps.hpp"):
        assert os.path.exists(os.path.join(ROOT, "pathtracer-0_amd", "csrc", "hip", f)), f


CLIENT = ('#include "pt_debug.h"\n#include "pt_rig_ik.h"\n#include <stddef.h>\n'
          "typedef char constraint_is_32_bytes[sizeof(pt_rig_ik_constraint) == 32 ? 1 : -1];\n"
          "typedef char goal_is_32_bytes[sizeof(pt_rig_ik_goal) == 32 ? 1 : -1];\n"
          "typedef char fields_lie_where_the_kernel_reads_them[offsetof(pt_rig_ik_constraint, joint) == 4 && offsetof(pt_rig_ik_constraint, flags) == 8 && "
          "offsetof(pt_rig_ik_constraint, axis) == 16 && offsetof(pt_rig_ik_goal, weight) == 12 && offsetof(pt_rig_ik_goal, pole) == 16 ? 1 : -1];\n"
          "int main(void) {\n"
          "    int (*a)(pt_rig*, const pt_rig_ik_constraint*, size_t) = pt_rig_ik_attach;\n"
          "    int (*g)(pt_rig*, const pt_rig_ik_goal*, size_t) = pt_rig_ik_goals;\n"
          "    int (*l)(pt_rig*, const float*, size_t, float*, size_t) = pt_rig_ik_locals;\n"
          "    int (*t)(struct pt_rig*, const float*, size_t, int, float*) = pt_debug_rig_ik_time;\n"
          "    pt_rig_ik_constraint c = {PT_RIG_IK_TWO_BONE, 4, PT_RIG_IK_POLE, 0, {0.0f, 0.0f, 1.0f}, 0.0f};\n"
          "    pt_rig_ik_goal y = {{1.0f, 2.0f, 3.0f}, 0.5f, {0.0f, 1.0f, 0.0f}, 0.0f};\n"
          "    return (a == NULL) + (g == NULL) + (l == NULL) + (t == NULL) + (c.joint != 4) + (y.weight != 0.5f) + (PT_RIG_IK_TWO_BONE != 0) + (PT_RIG_IK_AIM != 1)\n"
          "           + (PT_RIG_IK_POLE != 1);\n}\n")


@pytest.mark.parametrize("cc, std, name", [("gcc", "-std=c99", "client.c"), ("g++", "-std=c++17", "client.cpp")], ids=["c99", "c++"])
def test_ik_header_compiles_as_c99_and_as_cpp_and_the_records_are_32_bytes(tmp_path, cc, std, name):
    src = tmp_path / name
    src.write_text(CLIENT)
    exe = str(tmp_path / "client")
    out = subprocess.run([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", exe + ".o"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr


def test_the_refusals_that_need_no_device(lib):
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.pt_rig_ik_attach.argtypes = [vp, vp, sz]
    lib.pt_rig_ik_goals.argtypes = [vp, vp, sz]
    lib.pt_rig_ik_locals.argtypes = [vp, vp, sz, vp, sz]
    lib.pt_debug_rig_ik_time.argtypes = [vp, vp, sz, ci, vp]
    lib.pt_last_error.restype = ctypes.c_char_p
    fake = ctypes.c_int(0)                                             # an address that is no live rig: never followed
    at = ctypes.addressof(fake)
    c, g = IM.pack_constraints([IM.two_bone(2)]), IM.pack_goals([IM.goal((1.0, 2.0, 3.0))])
    loc, out, best = np.ones(36, f32), np.zeros(36, f32), ctypes.c_float(-2.0)
    for rig in (None, at):                                             # null, and an address that is no live rig
        assert lib.pt_rig_ik_attach(rig, c.ctypes.data, 32) == -1 and lib.pt_last_error() == b"pt_rig_ik_attach: null or destroyed rig"
        assert lib.pt_rig_ik_attach(rig, None, 31) == -1 and lib.pt_last_error() == b"pt_rig_ik_attach: null or destroyed rig"
        assert lib.pt_rig_ik_goals(rig, g.ctypes.data, 32) == -1 and lib.pt_last_error() == b"pt_rig_ik_goals: null or destroyed rig"
        assert lib.pt_rig_ik_goals(rig, None, 0) == -1 and lib.pt_last_error() == b"pt_rig_ik_goals: null or destroyed rig"
        assert lib.pt_rig_ik_locals(rig, loc.ctypes.data, 144, out.ctypes.data, 144) == -1 and lib.pt_last_error() == b"pt_rig_ik_locals: null or destroyed rig"
        assert lib.pt_debug_rig_ik_time(rig, loc.ctypes.data, 144, 1, ctypes.addressof(best)) == -1 and lib.pt_last_error() == b"pt_debug_rig_ik_time: bad argument"
    assert best.value == -2.0 and not out.any()


def test_the_python_layer_declares_the_ik_calls_and_packs_their_records(pt):
    from pathtracer_0_amd import renderer
    import inspect
    L = renderer.lib()
    for name, n in dict(pt_rig_ik_attach=3, pt_rig_ik_goals=3, pt_rig_ik_locals=5, pt_debug_rig_ik_time=5).items():
        assert len(getattr(L, name).argtypes) == n, name
    for name, params in dict(ik=["constraints"], ik_goals=["goals"], ik_locals=["locals"]).items():
        assert list(inspect.signature(getattr(renderer.Rig, name)).parameters)[1:] == params, name
    assert renderer.RIG_IK_CONSTRAINT.itemsize == 32 and renderer.RIG_IK_GOAL.itemsize == 32
    assert renderer.RIG_IK_CONSTRAINT == IM.CONSTRAINT and renderer.RIG_IK_GOAL == IM.GOAL      # the tests' packers lay the records out the same way
    c = renderer.rig_ik_constraints([("two_bone", 4, True), dict(kind="aim", joint=2, axis=(0.0, 0.6, 0.8)), (0, 7)])
    assert c["kind"].tolist() == [0, 1, 0] and c["joint"].tolist() == [4, 2, 7] and c["flags"].tolist() == [1, 0, 0] and np.array_equal(c["axis"][1], np.array([0.0, 0.6, 0.8], f32))
    assert c.tobytes() == IM.pack_constraints([IM.two_bone(4, True), IM.aim(2, (0.0, 0.6, 0.8)), IM.two_bone(7)]).tobytes()
    g = renderer.rig_ik_goals([((1.0, 2.0, 3.0),), dict(target=(0.0, 0.0, 1.0), weight=0.25, pole=(4.0, 5.0, 6.0))])
    assert g["weight"].tolist() == [1.0, 0.25] and g["pole"][1].tolist() == [4.0, 5.0, 6.0] and g["target"][0].tolist() == [1.0, 2.0, 3.0]
    assert g.tobytes() == IM.pack_goals([IM.goal((1.0, 2.0, 3.0)), IM.goal((0.0, 0.0, 1.0), 0.25, (4.0, 5.0, 6.0))]).tobytes()
    assert np.array_equal(renderer.rig_ik_goals(g), g) and renderer.rig_ik_constraints([]).nbytes == 0
    with pytest.raises(ValueError):
        renderer.rig_ik_constraints([dict(kind="aim")])
    with pytest.raises(ValueError):
        renderer.rig_ik_goals([dict(weight=1.0)])


def test_the_workload(pt):
    from pathtracer_0_amd import renderer
    m9, m8 = pt.scenes.m9_reaching(3), pt.scenes.m8_mixed(3)
    wl, parent, inv_bind, clips, cons, goals = m9[0], m9[3], m9[4], m9[5], m9[8], m9[9]
    assert wl.name == "M9" and np.array_equal(wl.buffers[3].view(np.uint32), m8[0].buffers[3].view(np.uint32)) and m9[7] == m8[7]      # M8's tube and layers
    c, g = renderer.rig_ik_constraints(cons), renderer.rig_ik_goals(goals)
    assert c["kind"].tolist() == [0] and c["joint"].tolist() == [4] and c["flags"].tolist() == [1] and parent[4] == 3 and parent[3] == 2
    assert not np.array_equal(g, renderer.rig_ik_goals(pt.scenes.m9_goals(wl, 4)))                           # a step is a function of its number
    model_c = [IM.two_bone(4, True)]
    for step in range(0, 20, 3):                                         # the target is within reach at every step: the tip follows it
        y = pt.scenes.m9_goals(wl, step)[0]
        model_g = [IM.goal(y["target"], y["weight"], y["pole"])]
        rest = clips[0][1][0]
        traces = []
        out = IM.ik_locals(parent, model_c, model_g, rest, traces=traces)
        assert traces[0]["written"] and traces[0]["dist"] < 0.95 * (traces[0]["l1"] + traces[0]["l2"])
        tip = IM.world64(parent, out)[4][:, 3]
        assert np.abs(tip - np.asarray(y["target"], f32)).max() < 1e-4, step
