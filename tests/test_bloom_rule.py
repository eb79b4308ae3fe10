"""CPU: the host-only step of pt_bloom, pt_tonemap_bloom and pt_tonemap_bloom_save_png (csrc/hip/pt_bloom_rule.hpp) through
tests/c/bloom_rule_check.cpp, a stand-alone program built twice with g++: plain, and under the address / undefined-behaviour sanitizers (which
must stay silent and agree).  What the calls refuse is stated here a second time, from the struct comments of include/pt_bloom.h: a grid around
every bound (the bound, its neighbours on both sides, -0, the smallest denormal, +-inf, NaN), every ordered pair of bad fields (the earlier
check answers), every check reached and every bound accepted.  The level table must be tests/_bloom_model.py's sizes for every W, H in 1 .. 70
and L in 1 .. 8, and norm and T the model's floats bit for bit."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import _bloom_model as BM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INF, NAN = float("inf"), float("nan")
DENORM = float(np.finfo(f32).smallest_subnormal)
FMAX = float(np.finfo(f32).max)
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
(OK, CTX, RULE, LEVELS, INTENSITY, THRESHOLD, SPREAD, SOURCE, IMAGE, EXPOSURE) = range(10)      # BloomCheck
FIELDS = ["levels", "intensity", "threshold", "spread", "source", "image", "exposure"]
GOOD = dict(BM.RULE, source=BM.SRC_FRAME, image=0, exposure=1.0)
TEXT = {CTX: "null context", RULE: "null bloom rule", LEVELS: "bloom.levels must lie in 1 .. 8", INTENSITY: "bloom.intensity must be finite and >= 0",
        THRESHOLD: "bloom.threshold must be finite and >= 0", SPREAD: "bloom.spread must lie in (0, 1]",
        SOURCE: "source must be PT_BLOOM_SRC_FRAME, PT_BLOOM_SRC_HOST or PT_BLOOM_SRC_FILTERED", EXPOSURE: "exposure must be finite and > 0"}
IMAGE_TEXT = {True: "PT_BLOOM_SRC_HOST needs rgba_in", False: "rgba_in must be NULL unless the source is PT_BLOOM_SRC_HOST"}


def _next(x, to):
    return float(np.nextafter(f32(x), f32(to)))


def _bits(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", x))[0]


def _r32(r):
    """the fields as the values that travel"""
    return {k: (v if k in ("levels", "source", "image") else float(f32(v))) for k, v in r.items()}


def expected(ctx, rule, r, with_exposure):
    """the first failing check, from the header's struct comments"""
    r = _r32(r)
    if not ctx:
        return CTX
    if not rule:
        return RULE
    if not 1 <= r["levels"] <= 8:
        return LEVELS
    if not (math.isfinite(r["intensity"]) and r["intensity"] >= 0):
        return INTENSITY
    if not (math.isfinite(r["threshold"]) and r["threshold"] >= 0):
        return THRESHOLD
    if not 0 < r["spread"] <= 1:
        return SPREAD
    if r["source"] not in (0, 1, 2):
        return SOURCE
    if (r["source"] == 1) != bool(r["image"]):
        return IMAGE
    if with_exposure and not (math.isfinite(r["exposure"]) and r["exposure"] > 0):
        return EXPOSURE
    return OK


SPECIAL = [0.0, -0.0, DENORM, -DENORM, INF, -INF, NAN, 3.0e38, -3.0e38]
AROUND_0 = [_next(0, -1), _next(0, 1)]
FLOAT_GRID = {
    "intensity": AROUND_0 + [0.05, FMAX] + SPECIAL,
    "threshold": AROUND_0 + [1.0, FMAX] + SPECIAL,
    "spread": AROUND_0 + [0.75, 1.0, _next(1, 0), _next(1, 2)] + SPECIAL,
    "exposure": AROUND_0 + [1.0, FMAX] + SPECIAL,
}
BAD = {"levels": 9, "intensity": -1.0, "threshold": NAN, "spread": 0.0, "source": 3, "image": 1, "exposure": -INF}      # image 1 with source FRAME


def cases():
    """(entry point, ctx, rule, fields, with exposure)"""
    out = []
    for who, we in (("pt_bloom", 1), ("pt_tonemap_bloom", 0), ("pt_tonemap_bloom_save_png", 0)):
        out += [(who, 0, 0, GOOD, we), (who, 0, 1, GOOD, we), (who, 1, 0, GOOD, we), (who, 1, 1, GOOD, we)]
        out.append((who, 0, 1, dict(GOOD, levels=0), we))              # a null context answers before a bad field
    for v in (INT_MIN, -1, 0, 1, 2, 8, 9, INT_MAX):
        out.append(("pt_bloom", 1, 1, dict(GOOD, levels=v), 1))
    for v in (INT_MIN, -1, 0, 1, 2, 3, INT_MAX):
        for image in (0, 1):
            out.append(("pt_tonemap_bloom", 1, 1, dict(GOOD, source=v, image=image), 0))
    for name, values in FLOAT_GRID.items():
        for v in values:
            out.append(("pt_bloom", 1, 1, dict(GOOD, **{name: v}), 1))
    out.append(("pt_tonemap_bloom", 1, 1, dict(GOOD, exposure=NAN), 0))      # the metering calls have no exposure argument to refuse
    for a in FIELDS:                                                   # every ordered pair of bad fields
        for b in FIELDS:
            if a != b:
                out.append(("pt_bloom", 1, 1, dict(GOOD, **{a: BAD[a], b: BAD[b]}), 1))
    return out


def _words(r):
    return f"{r['levels']} {_bits(r['intensity'])} {_bits(r['threshold'])} {_bits(r['spread'])} {r['source']} {r['image']}"


def number_cases():
    rng = np.random.default_rng(1618)
    norms = [(s, L) for L in range(1, 9) for s in (1.0, 0.5, 0.75, 0.3, DENORM, _next(1, 0), 1e-20, float(f32(rng.random())))]
    ts = [(0.0, 1.0), (1.0, 1.0), (1.0, 0.18), (1.0, DENORM), (DENORM, FMAX), (FMAX, DENORM), (0.0, DENORM), (3.0, FMAX), (0.7, 2.0 ** -10), (0.7, 2.0 ** 10)]
    ts += [(float(f32(10 ** rng.uniform(-3, 3))), float(f32(10 ** rng.uniform(-3, 3)))) for _ in range(100)]
    return norms, ts


def _build(tmp, name, extra):
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "c", "bloom_rule_check.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr      # no warning either
    return exe


SHAPES = [(W, H, L) for W in range(1, 71) for H in range(1, 71) for L in range(1, 9)]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bloom_rule")
    path = str(tmp / "requests.txt")
    todo = cases()
    norms, ts = number_cases()
    with open(path, "w") as f:
        for who, ctx, rule, r, we in todo:
            f.write(f"C {who} {ctx} {rule} {_words(r)} {we} {_bits(r['exposure'])}\n")
        for W, H, L in SHAPES:
            f.write(f"P {W} {H} {L}\n")
        for s, L in norms:
            f.write(f"N {_bits(s)} {L}\n")
        for t, e in ts:
            f.write(f"T {_bits(t)} {_bits(e)}\n")
    got = []
    for exe in (_build(tmp, "check_plain", []), _build(tmp, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0 and run.stderr == "", (exe, run.returncode, run.stderr[-2000:])
        got.append(run.stdout.splitlines())
    assert got[0] == got[1] and len(got[0]) == len(todo) + len(SHAPES) + len(norms) + len(ts)
    lines = got[0]
    a, b, c = len(todo), len(todo) + len(SHAPES), len(todo) + len(SHAPES) + len(norms)
    return todo, [line.split(" ", 2) for line in lines[:a]], lines[a:b], norms, lines[b:c], ts, lines[c:]


def test_every_call_answers_as_the_header_says(answers):
    todo, got = answers[:2]
    for (who, ctx, rule, r, we), (code, which, text) in zip(todo, got):
        want = expected(ctx, rule, r, we)
        assert int(which) == want, (who, ctx, rule, r, which, text)
        if want == OK:
            assert int(code) == 0 and text == "", (who, r, text)
        else:
            words = IMAGE_TEXT[r["source"] == 1] if want == IMAGE else TEXT[want]
            assert int(code) == -1 and text == who + ": " + words, (who, r, text)      # PT_ERR_ARG, under the caller's name


def test_every_check_is_reached_and_every_bound_is_accepted(answers):
    todo, got = answers[:2]
    assert {int(which) for _, which, _ in got} == set(range(10))
    accepted = [_r32(r) for (who, ctx, rule, r, we), (code, which, text) in zip(todo, got) if int(which) == OK and we]
    bounds = (("levels", (1, 8)), ("intensity", (0.0, -0.0, FMAX)), ("threshold", (0.0, -0.0, FMAX)), ("spread", (DENORM, 1.0)), ("exposure", (DENORM, FMAX)))
    for name, values in bounds:
        for v in values:
            assert any(r[name] == v and math.copysign(1, r[name]) == math.copysign(1, v) for r in accepted), (name, v)
    ok = [(r["source"], r["image"]) for (who, ctx, rule, r, we), (code, which, text) in zip(todo, got) if int(which) == OK]
    assert set(ok) == {(0, 0), (1, 1), (2, 0)}                         # each source with the image that fits it


def test_an_ordered_pair_answers_as_the_earlier_field(answers):
    todo, got = answers[:2]
    pairs = 0
    for (who, ctx, rule, r, we), (code, which, text) in zip(todo, got):
        bad = [i for i, n in enumerate(FIELDS) if (r[n] == BAD[n] if n in ("levels", "source", "image") else _bits(float(r[n])) == _bits(float(BAD[n])))]
        if who == "pt_bloom" and ctx and rule and len(bad) == 2:
            pairs += 1
            # (a bad source makes "an image with FRAME" no refusal of its own: SOURCE answers, which is the earlier field)
            assert int(which) == LEVELS + bad[0], (r, which)
    assert pairs == 42


def test_the_level_table_is_the_models(answers):
    lines = answers[2]
    for (W, H, L), line in zip(SHAPES, lines):
        v = [int(x) for x in line.split()]
        sizes = BM.sizes(W, H, L)[1:]
        offsets = np.concatenate([[0], np.cumsum([w * h for w, h in sizes])])
        want = [L] + [x for (w, h), o in zip(sizes, offsets) for x in (w, h, int(o))] + [int(offsets[-1])]
        assert v == want, (W, H, L, line)
    big = BM.sizes(1920, 1080, 8)[1:]
    assert big[0] == (960, 540) and big[-1] == (8, 5) and 10.5e6 < 16 * sum(w * h for w, h in big[:6]) < 11.5e6      # about 11 MB at 1080p


def test_norm_and_T_equal_the_model_bit_for_bit(answers):
    norms, got_n, ts, got_t = answers[3:]
    for (s, L), word in zip(norms, got_n):
        assert word == _bits(float(BM.norm(s, L))), (s, L, word)
    for (t, e), word in zip(ts, got_t):
        assert word == _bits(float(BM.threshold(t, e))), (t, e, word)
    assert _bits(INF) in got_t and _bits(0.0) in got_t                # the quotient may overflow (nothing blooms) and may be 0
