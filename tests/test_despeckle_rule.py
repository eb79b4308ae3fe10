"""CPU: what pt_despeckle and pt_despeckle_frame refuse in their arguments (csrc/hip/pt_despeckle_rule.hpp) through tests/c/despeckle_rule_check.cpp,
a stand-alone program built twice with g++: plain, and under the address / undefined-behaviour sanitizers (which must stay silent and agree).
The expectations are stated here a second time, from the struct comments of include/pt_despeckle.h: a grid around every bound (the bound, its
neighbours on both sides, -0, the smallest denormal, +-inf, NaN), every ordered pair of bad fields (the earlier check answers), every text
reached and every bound accepted."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INF, NAN = float("inf"), float("nan")
DENORM = float(np.finfo(f32).smallest_subnormal)
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
OK, CTX, RULE, RADIUS, SIGMAS, MIN_TAPS, OWN_Z, NORMAL_TOL, MIN_LUM = range(9)      # DespeckleCheck
FIELDS = ["radius", "sigmas", "min_taps", "own_z", "normal_tol", "min_lum"]
GOOD = dict(radius=2, sigmas=2.0, min_taps=4, own_z=3.0, normal_tol=0.9, min_lum=0.0)
TEXT = {CTX: "null context", RULE: "null rule", RADIUS: "rule.radius must be 1 .. 3", SIGMAS: "rule.sigmas must be finite and >= 0",
        MIN_TAPS: "rule.min_taps must be 2 .. (2*radius + 1)^2 - 1 = ", OWN_Z: "rule.own_z must be > 0 (+inf turns the test off)",
        NORMAL_TOL: "rule.normal_tol must lie in [-1, 1]", MIN_LUM: "rule.min_lum must be finite and >= 0"}


def _next(x, to):
    return float(np.nextafter(f32(x), f32(to)))


def _bits(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", x))[0]


def expected(ctx, rule, r):
    """the first failing check, from the header's struct comments"""
    if not ctx:
        return CTX
    if not rule:
        return RULE
    if not 1 <= r["radius"] <= 3:
        return RADIUS
    if not (math.isfinite(r["sigmas"]) and r["sigmas"] >= 0):
        return SIGMAS
    if not 2 <= r["min_taps"] <= (2 * r["radius"] + 1) ** 2 - 1:
        return MIN_TAPS
    if not r["own_z"] > 0:                                            # +inf is accepted; a NaN is not > 0
        return OWN_Z
    if not -1 <= r["normal_tol"] <= 1:
        return NORMAL_TOL
    if not (math.isfinite(r["min_lum"]) and r["min_lum"] >= 0):
        return MIN_LUM
    return OK


SPECIAL = [0.0, -0.0, DENORM, -DENORM, INF, -INF, NAN, 3.0e38, -3.0e38]
FLOAT_GRID = {
    "sigmas": [_next(0, -1), _next(0, 1), 2.0, float(np.finfo(f32).max)] + SPECIAL,
    "own_z": [_next(0, -1), _next(0, 1), 3.0, float(np.finfo(f32).max)] + SPECIAL,
    "normal_tol": [-1.0, _next(-1, -2), _next(-1, 0), 1.0, _next(1, 2), _next(1, 0)] + SPECIAL,
    "min_lum": [_next(0, -1), _next(0, 1), 0.25, float(np.finfo(f32).max)] + SPECIAL,
}
BAD = {"radius": 0, "sigmas": -1.0, "min_taps": 1, "own_z": 0.0, "normal_tol": 1.5, "min_lum": NAN}


def cases():
    out = []
    for who in ("pt_despeckle", "pt_despeckle_frame"):
        out += [(who, 0, 0, GOOD), (who, 0, 1, GOOD), (who, 1, 0, GOOD), (who, 1, 1, GOOD)]
        out.append((who, 0, 1, dict(GOOD, radius=0)))                 # a null context answers before a bad field
    for radius in (INT_MIN, -1, 0, 1, 2, 3, 4, INT_MAX):
        out.append(("pt_despeckle", 1, 1, dict(GOOD, radius=radius)))
    for radius, top in ((1, 8), (2, 24), (3, 48)):                    # min_taps' upper bound follows the radius
        for taps in (INT_MIN, -1, 0, 1, 2, 3, top - 1, top, top + 1, INT_MAX):
            out.append(("pt_despeckle_frame", 1, 1, dict(GOOD, radius=radius, min_taps=taps)))
    for name, values in FLOAT_GRID.items():
        for v in values:
            out.append(("pt_despeckle", 1, 1, dict(GOOD, **{name: v})))
    for a in FIELDS:                                                  # every ordered pair of bad fields
        for b in FIELDS:
            if a != b:
                out.append(("pt_despeckle_frame", 1, 1, dict(GOOD, **{a: BAD[a], b: BAD[b]})))
    return out


def _build(tmp, name, extra):
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "c", "despeckle_rule_check.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr      # no warning either
    return exe


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("despeckle_rule")
    path = str(tmp / "calls.txt")
    todo = cases()
    with open(path, "w") as f:
        for who, ctx, rule, r in todo:
            f.write(f"{who} {ctx} {rule} {r['radius']} {_bits(r['sigmas'])} {r['min_taps']} {_bits(r['own_z'])} {_bits(r['normal_tol'])} {_bits(r['min_lum'])}\n")
    got = []
    for exe in (_build(tmp, "check_plain", []), _build(tmp, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0 and run.stderr == "", (exe, run.returncode, run.stderr[-2000:])
        got.append(run.stdout.splitlines())
    assert got[0] == got[1] and len(got[0]) == len(todo)
    return todo, [line.split(" ", 2) for line in got[0]]


def test_every_call_answers_as_the_header_says(answers):
    todo, got = answers
    for (who, ctx, rule, r), (code, which, text) in zip(todo, got):
        want = expected(ctx, rule, r)
        assert int(which) == want, (who, ctx, rule, r, which, text)
        if want == OK:
            assert int(code) == 0 and text == "", (who, r, text)
        else:
            assert int(code) == -1 and text.startswith(who + ": " + TEXT[want]), (who, r, text)      # PT_ERR_ARG, under the caller's name
            if want == MIN_TAPS:
                assert text == who + ": " + TEXT[want] + str((2 * r["radius"] + 1) ** 2 - 1)


def test_every_text_is_reached_and_every_bound_is_accepted(answers):
    todo, got = answers
    reached = {int(which) for _, which, _ in got}
    assert reached == set(range(9))
    accepted = [r for (who, ctx, rule, r), (code, which, text) in zip(todo, got) if int(which) == OK]
    for name, values in (("radius", (1, 3)), ("sigmas", (0.0, -0.0, float(np.finfo(f32).max))), ("own_z", (DENORM, INF)),
                         ("normal_tol", (-1.0, 1.0)), ("min_lum", (0.0, -0.0, float(np.finfo(f32).max)))):
        for v in values:
            assert any(r[name] == v and math.copysign(1, r[name]) == math.copysign(1, v) for r in accepted), (name, v)
    for radius, top in ((1, 8), (2, 24), (3, 48)):
        for taps in (2, top):
            assert any(r["radius"] == radius and r["min_taps"] == taps for r in accepted), (radius, taps)


def test_an_ordered_pair_answers_as_the_earlier_field(answers):
    todo, got = answers
    pairs = 0
    for (who, ctx, rule, r), (code, which, text) in zip(todo, got):
        bad = [i for i, n in enumerate(FIELDS) if _bits(float(r[n])) == _bits(float(BAD[n]))]
        if ctx and rule and len(bad) == 2:
            pairs += 1
            assert int(which) == RADIUS + bad[0], (r, which)
    assert pairs == 30
