"""CPU: the host-only half of the in-place move (csrc/hip/pt_scene_move.hpp; include/pt_move.h) through tests/c/scene_move_check.cpp, a
stand-alone program built with g++ under the address and undefined-behaviour sanitizers (which must stay silent on every case).

Every case lays out the old scene, patches the layout with applyMove — new triangles and the binding 10 that the numpy model of the refit
(tests/_refit_model.py) gives for them — and holds the result to layoutScene on the new buffers: every array byte for byte, every count and mode."""
import os
import struct
import subprocess

import numpy as np
import pytest

import _move_cases as MC
import _refit_cases as RC
import _refit_model as RM
from test_scene_layout import one_ellipsoid, replace, write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scene_move")
    exe = str(tmp / "move_check_san")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "c", "scene_move_check.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    return tmp, exe


def run(program, name, buffers, textures, tris, data, ellip=None, **options):
    tmp, exe = program
    scene, move = str(tmp / (name + ".scene")), str(tmp / (name + ".move"))
    write_scene(scene, buffers, textures, **options)
    with open(move, "wb") as f:
        for a in (tris, data, np.zeros(0, f32) if ellip is None else ellip):
            a = np.ascontiguousarray(a, f32)
            f.write(struct.pack("<Q", a.size)); f.write(a.tobytes())
    r = subprocess.run([exe, scene, move], capture_output=True, text=True, timeout=300)
    os.remove(scene); os.remove(move)
    assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
    out = {}
    for line in r.stdout.splitlines():
        k, _, v = line.partition(" ")
        out[k] = v
    return out


def patched_equals_fresh(got, tag):
    assert got["rc"] == "0" and got["slow"] == "0" and got["order_same"] == "1", (tag, got)
    assert got["new_rc"] == "0", (tag, got)
    assert got["differs"] == "", (tag, got["differs"])
    assert got["ordered_as_found"] == "1" and got["digest_old"] == got["digest_new"], (tag, got)


# bfs_nodes: 0 (depth-first from the roots' children on), 3, 5 (the third level of a single tree holds records 3..6: cut in two), all
OPTION_SETS = [("default", {})] + [(f"layout{v}", dict(asmNodeLayout=v)) for v in (0, 1)] + [(f"bfs{v}", dict(bfsNodes=v)) for v in (0, 3, 5)] + \
              [("nocull", dict(asmNoRootCull=1)), ("layout0-bfs5-nocull", dict(asmNodeLayout=0, bfsNodes=5, asmNoRootCull=1)),
               ("layout1-bfs3", dict(asmNodeLayout=1, bfsNodes=3))]
EXTRA = [f"soup{n}" for n, _, _ in RC.SOUPS] + ["ladder60", "chain60", "loose", "objects70", "leafroot", "emptyleaf", "hand"]


@pytest.mark.parametrize("variant,options", OPTION_SETS, ids=[v for v, _ in OPTION_SETS])
@pytest.mark.parametrize("name", EXTRA)
def test_patch_equals_layout_on_soups_ladders_and_hand_made_scenes(pt, program, name, variant, options):
    b = MC.scenes(pt)[name]
    tris, data = MC.moved(pt, name)
    got = run(program, f"{name}-{variant}", b, MC.SKY, tris, data, **options)
    patched_equals_fresh(got, (name, variant))
    if name == "objects70":
        assert got["numObj"] == "70" and got["asmGroupShift"] == "1"
        pads = got["group_pads"].split()
        assert pads[:35] == ["1" if options.get("asmNoRootCull") else "0"] * 35       # inner roots over tight refit boxes: cullable unless switched off
    if name == "leafroot":
        pads = got["group_pads"].split()
        assert got["numObj"] == "10" and pads[9] == "1" and (options.get("asmNoRootCull") or pads[:9] == ["0"] * 9)
    if name == "emptyleaf":
        assert got["anyEmpty"] == "1" and got["asmWhyNot"] == "a leaf without triangles"
    if name == "chain60":
        assert got["nInner"] == "60"
    if name == "ladder60":
        assert int(got["nInner"]) >= 30


@pytest.mark.parametrize("name", ["ladder", "chain256"])
def test_the_long_ladders_are_no_scene_a_context_can_hold(pt, program, name):
    """180 and 256 heights: the layout step refuses them (the reference's 64-entry stack), so there is nothing to move"""
    b = MC.scenes(pt)[name]
    tris, data = MC.moved(pt, name)
    got = run(program, name, b, MC.SKY, tris, data)
    assert got == {"rc": "-4", "err": "BVH too deep for the reference's `int stack[64]` (frag.glsl:465)"}


def test_a_vertex_at_infinity_gives_the_nan_edges_the_layout_gives(pt, program):
    b = MC.scenes(pt)["hand"]
    tris, data = MC.move_of(b, MC.infinite_vertex(b[3]))
    assert np.isinf(data).any()
    got = run(program, "hand-inf", b, MC.SKY, tris, data)
    patched_equals_fresh(got, "inf")
    assert int(got["tri_nan"]) >= 1


def test_foreign_unordered_boxes_in_80_byte_records_take_the_slow_path(pt, program):
    b = MC.scenes(pt)["unordered80"]
    tris, data = MC.moved(pt, "unordered80")
    for options, slow in ((dict(asmNodeLayout=0), "1"), ({}, "1"), (dict(asmNodeLayout=1), "0")):
        got = run(program, "unordered", b, MC.SKY, tris, data, **options)
        assert got["rc"] == "0" and got["slow"] == slow and got["boxesOrdered"] == "0" and got["order_same"] == "1", (options, got)
        if slow == "1":
            assert "differs" not in got                              # applyMove was not called
        else:
            patched_equals_fresh(got, "unordered at stride 64")


WORKLOAD_OPTIONS = [("default", {}), ("layout0-bfs5", dict(asmNodeLayout=0, bfsNodes=5)), ("layout1-bfs0-nocull", dict(asmNodeLayout=1, bfsNodes=0, asmNoRootCull=1)),
                    ("bfs3", dict(bfsNodes=3))]
_moves = {}


def workload_move(pt, name):
    if name not in _moves:
        b = RC.workloads(pt)[name]
        _moves[name] = MC.move_of(b, RC.perturbed(b[3], 11, 0.01))
    return _moves[name]


@pytest.mark.parametrize("name", list(RC.WORKLOADS))
def test_patch_equals_layout_on_the_workloads(pt, program, name):
    wl = RC.workload(pt, name)
    b, tex = MC.workload_inputs(wl)
    tris, data = workload_move(pt, name)
    for variant, options in WORKLOAD_OPTIONS:
        got = run(program, f"{name}-{variant}", b, tex, tris, data, **options)
        patched_equals_fresh(got, (name, variant))
    if name == "C6":
        assert got["numObj"] == "64" and got["asmGroupShift"] == "0"


@pytest.mark.parametrize("step", [1, 4, 8])
def test_m1_from_the_rest_pose_with_its_moved_ellipsoid(pt, program, step):
    """the normals (shading records) and binding 7 change too"""
    rest, wl = pt.scenes.m1_moving(0), pt.scenes.m1_refit(step)
    b, tex = MC.workload_inputs(rest)
    data = RM.refit_buffers(wl.buffers)[0]
    assert not np.array_equal(wl.buffers[7], rest.buffers[7]) and not np.array_equal(wl.buffers[3].reshape(-1, 40)[:, 12:36], rest.buffers[3].reshape(-1, 40)[:, 12:36])
    for variant, options in WORKLOAD_OPTIONS:
        for ellip in (wl.buffers[7], None):
            got = run(program, f"M1-{step}-{variant}", b, tex, wl.buffers[3], data, ellip, **options)
            if ellip is not None:
                assert got["ellip_rc"] == "0" and got["ellip_patchable"] == "1"
            patched_equals_fresh(got, (step, variant, ellip is not None))


def test_binding_7_that_changes_a_count_or_a_material_is_not_patchable_and_a_bad_one_is_refused(pt, program):
    rest = pt.scenes.m1_moving(0)
    b, tex = MC.workload_inputs(rest)
    tris, data = rest.buffers[3], RM.refit_buffers(rest.buffers)[0]
    e = rest.buffers[7].copy()
    assert e[0] == 1.0 and e.size == 12
    other = e.copy(); other[11] = 0.0 if e[11] != 0.0 else 1.0
    cases = [(other, "0", "0"), (np.array([0.0], f32), "0", "0"), (replace((b, tex), 7, e)[0][7][:11], "-4", "0"), (one_ellipsoid(1000.0), "-4", "0"),
             (one_ellipsoid(float("nan")), "-4", "0"), (e, "0", "1")]
    for ellip, rc, patchable in cases:
        got = run(program, "M1-ellip", b, tex, tris, data, ellip)
        assert got["ellip_rc"] == rc and got["ellip_patchable"] == patchable, (ellip, got)
