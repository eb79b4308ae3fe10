"""CPU: the host-only step of include/pt_pose.h (csrc/hip/pt_pose_rule.hpp) through tests/c/pose_rule_check.cpp, a stand-alone program built twice
with g++: plain, and under the address / undefined-behaviour sanitizers (which must stay silent and agree).  What the calls refuse is stated here
a second time, from the header: the bounds and their neighbours, every ordered pair of bad fields (the earlier check answers), every check
reached.  The C++ statement of the rule must equal tests/_pose_model.py bit for bit; and the model must differ from a fused and from a binary64
evaluation on a chosen input, so that the comparison can tell them apart."""
import os
import subprocess

import numpy as np
import pytest

import _pose_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
(OK, NULL, PART_BYTES, N_PARTS, PART_ID, POSE, FOREIGN, XFORMS, XFORM_BYTES, ELLIP_BYTES, TRIS_OUT, TRI_BYTES) = range(12)      # PoseCheck
TEXT = {NULL: "null ctx, tri_part or out", PART_BYTES: "part_bytes != n_tris * 4", N_PARTS: "n_parts must lie in 0 .. 65536",
        PART_ID: "a part id outside [-1, n_parts)", POSE: "null or destroyed pose", FOREIGN: "the pose was created on another context",
        XFORMS: "null xforms with n_parts > 0", XFORM_BYTES: "xform_bytes != n_parts * 96", ELLIP_BYTES: "ellip_bytes must be a multiple of 4 bytes",
        TRIS_OUT: "null tris_out", TRI_BYTES: "tri_bytes != n_tris * 160"}
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


# ---- the header's order, stated a second time

def expect_create(r):
    if not (r["ctx"] and r["part"] and r["out"]):
        return NULL
    if r["part_bytes"] != 4 * len(r["ids"]):
        return PART_BYTES
    if not 0 <= r["n_parts"] <= 65536:
        return N_PARTS
    if any(not -1 <= i < r["n_parts"] for i in r["ids"]):
        return PART_ID
    return OK


def expect_geometry(r):
    if not r["ctx"]:
        return NULL
    if not r["live"]:
        return POSE
    if not r["own"]:
        return FOREIGN
    if not r["xf"] and r["n_parts"] > 0:
        return XFORMS
    if r["xform_bytes"] != 96 * r["n_parts"]:
        return XFORM_BYTES
    if r["ellip"] and r["ellip_bytes"] % 4:
        return ELLIP_BYTES
    return OK


def expect_triangles(r):
    if not r["live"]:
        return POSE
    if not r["xf"] and r["n_parts"] > 0:
        return XFORMS
    if r["xform_bytes"] != 96 * r["n_parts"]:
        return XFORM_BYTES
    if not r["out"]:
        return TRIS_OUT
    if r["tri_bytes"] != 160 * r["n_tris"]:
        return TRI_BYTES
    return OK


C_GOOD = dict(ctx=1, part=1, out=1, part_bytes=12, n_parts=3, ids=[-1, 0, 2])
C_BAD = [("ctx", 0), ("part_bytes", 8), ("n_parts", 65537), ("ids", [-1, 0, 70000])]      # in the order of the checks (70000 is out of range under any n_parts)
G_GOOD = dict(ctx=1, live=1, own=1, xf=1, xform_bytes=288, n_parts=3, ellip=1, ellip_bytes=48)
G_BAD = [("ctx", 0), ("live", 0), ("own", 0), ("xf", 0), ("xform_bytes", 287), ("ellip_bytes", 46)]
T_GOOD = dict(live=1, xf=1, xform_bytes=288, n_parts=3, out=1, tri_bytes=480, n_tris=3)
T_BAD = [("live", 0), ("xf", 0), ("xform_bytes", 96), ("out", 0), ("tri_bytes", 479)]


def cases():
    out = []
    for kind, good, bad in (("C", C_GOOD, C_BAD), ("G", G_GOOD, G_BAD), ("T", T_GOOD, T_BAD)):
        out.append((kind, dict(good)))
        for k, v in bad:
            out.append((kind, dict(good, **{k: v})))
        for a, va in bad:                                            # every ordered pair of bad fields
            for b, vb in bad:
                if a != b:
                    out.append((kind, dict(good, **{a: va, b: vb})))
    # pt_pose_create: each null alone; the bounds and their neighbours
    for k in ("ctx", "part", "out"):
        out.append(("C", dict(C_GOOD, **{k: 0})))
    for pb in (0, 11, 13, 16):
        out.append(("C", dict(C_GOOD, part_bytes=pb)))
    for n in (INT_MIN, -1, 0, 1, 65535, 65536, 65537, INT_MAX):
        out.append(("C", dict(C_GOOD, n_parts=n, ids=[-1, -1, -1])))
    for n_parts in (0, 1, 3, 65536):
        for i in (INT_MIN, -2, -1, 0, n_parts - 1, n_parts, n_parts + 1, INT_MAX):
            out.append(("C", dict(C_GOOD, n_parts=n_parts, ids=[-1, i, -1])))
            out.append(("C", dict(C_GOOD, n_parts=n_parts, ids=[-1, -1, i])))      # (the last id is read too)
    out.append(("C", dict(C_GOOD, part_bytes=0, ids=[], n_parts=0)))              # a scene without triangles, a pose without parts
    # pt_pose_geometry / pt_pose_triangles: n_parts = 0 needs no matrices; the byte counts around the right one
    for kind, good in (("G", G_GOOD), ("T", T_GOOD)):
        out.append((kind, dict(good, n_parts=0, xf=0, xform_bytes=0)))
        out.append((kind, dict(good, n_parts=0, xf=1, xform_bytes=0)))
        out.append((kind, dict(good, n_parts=0, xf=0, xform_bytes=96)))
        for n_parts in (1, 3, 65536):
            for d in (-96, -4, -1, 0, 1, 4, 96):
                out.append((kind, dict(good, n_parts=n_parts, xform_bytes=96 * n_parts + d)))
    for eb in (0, 1, 2, 3, 4, 5, 44, 47, 48):
        out.append(("G", dict(G_GOOD, ellip_bytes=eb)))
        out.append(("G", dict(G_GOOD, ellip=0, ellip_bytes=eb)))                  # no ellipsoids given: their byte count is not looked at
    for n_tris in (0, 1, 3):
        for d in (-160, -1, 0, 1, 160):
            if 160 * n_tris + d >= 0:
                out.append(("T", dict(T_GOOD, n_tris=n_tris, tri_bytes=160 * n_tris + d)))
    return out


def _line(kind, r):
    if kind == "C":
        return f"C {r['ctx']} {r['part']} {r['out']} {r['part_bytes']} {r['n_parts']} {len(r['ids'])} " + " ".join(str(i) for i in r["ids"])
    if kind == "G":
        return f"G {r['ctx']} {r['live']} {r['own']} {r['xf']} {r['xform_bytes']} {r['n_parts']} {r['ellip']} {r['ellip_bytes']}"
    return f"T {r['live']} {r['xf']} {r['xform_bytes']} {r['n_parts']} {r['out']} {r['tri_bytes']} {r['n_tris']}"


def _words(a):
    return " ".join("%08x" % w for w in np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32))


def rule_cases():
    """(rest, parts, xforms)"""
    rng = np.random.RandomState(11)
    out = []
    for n, n_parts in ((1, 1), (7, 3), (64, 5)):                     # random triangles, random matrices
        out.append((rng.normal(0, 3, 40 * n).astype(f32), rng.randint(-1, n_parts, n).astype(np.int32), rng.normal(0, 2, 24 * n_parts).astype(f32)))
    n = 48                                                            # +-0, denormals, +-inf, 3e38 under rotations and under special matrices
    out.append((PM.special_triangles(n), PM.parts_mod4(n), PM.matrices(3)))
    X = rng.normal(0, 1, (3, 24)).astype(f32)
    X[0, :21] = PM.SPECIAL[rng.randint(0, PM.SPECIAL.size, 21)]
    X[1, [0, 5, 10]] = (0.0, -0.0, 1e-45)
    out.append((PM.special_triangles(n, 4), PM.parts_mod4(n), X.reshape(-1)))
    out.append((rng.normal(0, 3, 40 * 5).astype(f32), np.full(5, -1, np.int32), PM.matrices(2)))      # part -1 rows unchanged
    out.append((rng.normal(0, 3, 40 * 5).astype(f32), np.full(5, -1, np.int32), np.zeros(0, f32)))    # n_parts = 0
    return out


def _build(tmp, name, extra):
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "c", "pose_rule_check.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr      # no warning either
    return exe


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pose_rule")
    path = str(tmp / "requests.txt")
    todo, rules = cases(), rule_cases()
    with open(path, "w") as f:
        for kind, r in todo:
            f.write(_line(kind, r) + "\n")
        for rest, parts, X in rules:
            f.write(f"R {parts.size} {X.size // 24} " + " ".join(str(int(p)) for p in parts) + " " + _words(rest) + " " + _words(X) + "\n")
    got = []
    for exe in (_build(tmp, "check_plain", []), _build(tmp, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0 and run.stderr == "", (exe, run.returncode, run.stderr[-2000:])
        got.append(run.stdout.splitlines())
    assert got[0] == got[1] and len(got[0]) == len(todo) + len(rules)
    return todo, [line.split(" ", 2) for line in got[0][:len(todo)]], rules, got[0][len(todo):]


EXPECT = {"C": expect_create, "G": expect_geometry, "T": expect_triangles}
WHO = {"C": "pt_pose_create", "G": "pt_pose_geometry", "T": "pt_pose_triangles"}


def test_every_call_answers_as_the_header_says(answers):
    todo, got = answers[:2]
    for (kind, r), (code, which, text) in zip(todo, got):
        want = EXPECT[kind](r)
        assert int(which) == want, (kind, r, which, text)
        if want == OK:
            assert int(code) == 0 and text == "", (kind, r, text)
        else:
            words = "null ctx" if (kind, want) == ("G", NULL) else TEXT[want]      # (pt_pose_geometry takes neither tri_part nor out)
            assert int(code) == -1 and text == WHO[kind] + ": " + words, (kind, r, text)      # PT_ERR_ARG, under the entry point's name


def test_every_check_is_reached_and_every_bound_is_accepted(answers):
    todo, got = answers[:2]
    assert {int(which) for _, which, _ in got} == set(range(12))
    ok = [(kind, r) for (kind, r), (code, which, text) in zip(todo, got) if int(which) == OK]
    assert {r["n_parts"] for kind, r in ok if kind == "C"} >= {0, 1, 65535, 65536}
    assert any(kind == "C" and r["n_parts"] == 65536 and 65535 in r["ids"] for kind, r in ok)
    assert any(kind == "C" and r["ids"] == [] for kind, r in ok)
    assert any(kind == "G" and r["n_parts"] == 0 and not r["xf"] for kind, r in ok) and any(kind == "T" and r["n_parts"] == 0 and not r["xf"] for kind, r in ok)
    assert any(kind == "G" and not r["ellip"] and r["ellip_bytes"] % 4 for kind, r in ok)
    assert any(kind == "T" and r["n_tris"] == 0 and r["tri_bytes"] == 0 for kind, r in ok)


def test_an_ordered_pair_answers_as_the_earlier_field(answers):
    todo, got = answers[:2]
    pairs = 0
    for (kind, r), (code, which, text) in zip(todo, got):
        good, bad = {"C": (C_GOOD, C_BAD), "G": (G_GOOD, G_BAD), "T": (T_GOOD, T_BAD)}[kind]
        if set(r) != set(good):
            continue
        wrong = [i for i, (k, v) in enumerate(bad) if r[k] == v]
        if len(wrong) == 2 and all(r[k] == good[k] for k in good if k not in [bad[i][0] for i in wrong]):
            pairs += 1
            first = {"C": [NULL, PART_BYTES, N_PARTS, PART_ID], "G": [NULL, POSE, FOREIGN, XFORMS, XFORM_BYTES, ELLIP_BYTES],
                     "T": [POSE, XFORMS, XFORM_BYTES, TRIS_OUT, TRI_BYTES]}[kind][wrong[0]]
            assert int(which) == first, (kind, r, which)
    assert pairs == 4 * 3 + 6 * 5 + 5 * 4


def test_the_cpp_rule_equals_the_model_bit_for_bit(answers):
    rules, lines = answers[2:]
    seen_special = False
    for (rest, parts, X), line in zip(rules, lines):
        got = np.array([int(w, 16) for w in line.split()], np.uint32)
        want = PM.pose(rest, parts, X).view(np.uint32)
        assert got.shape == want.shape and np.array_equal(got, want), (parts.size, X.size // 24, int((got != want).sum()))
        static = np.repeat(parts < 0, 40)
        assert np.array_equal(got[static], np.ascontiguousarray(rest, f32).view(np.uint32)[static])      # part -1: the rest pose's bits
        keep = np.ones(40, bool); keep[[0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14, 16, 17, 18, 20, 21, 22]] = False
        assert np.array_equal(got.reshape(-1, 40)[:, keep], np.ascontiguousarray(rest, f32).view(np.uint32).reshape(-1, 40)[:, keep])
        seen_special = seen_special or bool(np.isnan(got.view(f32)).any())
    assert seen_special                                               # inf * 0 and inf - inf did occur


def test_the_header_s_notes_on_the_identity():
    """an identity M is not a no-op: -0.0 becomes +0.0 and an infinite coordinate a NaN; part -1 leaves both alone"""
    t = np.ones(80, f32); t[0] = -0.0; t[4] = np.inf; t[40] = -0.0; t[44] = np.inf      # vertex 1: x = -0; vertex 2: x = inf
    X = PM.records(np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1))
    out = PM.pose(t, np.array([0, -1], np.int32), X)
    assert out[:1].view(np.uint32)[0] == 0 and out[1] == 1.0 and out[4] == np.inf and np.isnan(out[5:7]).all()      # rows 1, 2: 0 * inf
    assert out[40:41].view(np.uint32)[0] == 0x80000000 and out[44] == np.inf and (out[45:47] == 1.0).all()


def test_the_model_is_neither_a_fused_nor_a_binary64_evaluation():
    """a rotation of a chosen triangle: on at least one float the model's rounded products differ from the fused chain and from binary64"""
    rng = np.random.RandomState(2)
    rest = rng.uniform(-5, 5, 40 * 8).astype(f32)
    parts = np.zeros(8, np.int32)
    X = PM.records(PM.rotation((1.0, 2.0, 3.0), 0.7, (0.1, -0.2, 0.3)))
    a, b, c = PM.pose(rest, parts, X), PM.pose_fma(rest, parts, X), PM.pose_f64(rest, parts, X)
    assert (a.view(np.uint32) != b.view(np.uint32)).any() and (a.view(np.uint32) != c.view(np.uint32)).any()
    assert np.allclose(a, c, rtol=0, atol=1e-5) and np.allclose(a, b, rtol=0, atol=1e-5)      # the same numbers up to rounding


def test_the_derived_normal_matrix_is_the_inverse_transpose_in_binary64():
    M = PM.rotation((0.0, 1.0, 0.0), 0.5, (1, 2, 3), scale=2.0)
    X = PM.records(M)
    assert X.shape == (1, 24) and np.array_equal(X[0, :12], M.reshape(12).astype(f32))
    assert np.array_equal(X[0, 12:21], np.linalg.inv(M[:, :3]).T.reshape(9).astype(f32)) and not X[0, 21:].any()
