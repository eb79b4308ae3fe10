"""The shading kernel's serial chain of memory round trips after the flag-dependent state groups were folded into one trip, read statically from
the compiled code (scripts/shade_tiers.py; hipcc, no GPU), against the figures of the commit before that change (tests/golden/shade_tiers_parent.json,
written by `scripts/shade_tiers.py --json` on that commit).

k_shade is latency bound at 7 waves per SIMD: a restructuring pays only if it removes round trips WITHOUT costing a wave, a spill or a tier in
any instantiation (profiles/REJECTED.md has the forms that did not)."""
import importlib.util
import json
import os
import shutil
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3 = "k_shade<3,false,false,false,false>"           # the variant bench.py's default workload runs

pytestmark = pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")


@pytest.fixture(scope="module")
def report():
    spec = importlib.util.spec_from_file_location("shade_tiers", os.path.join(ROOT, "scripts", "shade_tiers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with tempfile.TemporaryDirectory() as d:
        return mod.report(open(mod.compile_asm(d)).read())


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(ROOT, "tests", "golden", "shade_tiers_parent.json")) as f:
        return json.load(f)


def test_c3_chain(report):
    v = report[C3]
    print(C3, v)
    assert v["tiers"] <= 14, v
    assert v["pre_barrier_trips"] <= 2, v           # (G2 G1 G0 H), then (G3 G5 J G4) under the job pull's barrier
    assert v["vgpr"] <= 72 and v["waves_per_simd"] >= 7, v
    assert v["scratch_bytes"] == 0, v


def test_no_instantiation_pays_for_it(report, parent):
    assert len(parent) == 28 and sorted(report) == sorted(parent)
    for name in sorted(parent):
        was, now = parent[name], report[name]
        print(name, was, now)
        assert now["waves_per_simd"] >= was["waves_per_simd"], (name, was, now)
        assert now["scratch_bytes"] <= was["scratch_bytes"], (name, was, now)
        assert now["tiers"] <= was["tiers"], (name, was, now)


def test_pre_barrier_trips_counts_round_trips():
    """the figure on hand-written code: a wait for a load that was already in flight during the previous trip is no new trip, a 4-byte load is
    not a state group, and nothing behind the first barrier counts"""
    spec = importlib.util.spec_from_file_location("shade_tiers", os.path.join(ROOT, "scripts", "shade_tiers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ld4, ld2, q = "\tglobal_load_dwordx4 v[0:3], v[4:5], off nt", "\tglobal_load_dwordx2 v[0:1], v[4:5], off", "\tglobal_load_dword v0, v[4:5], off"
    w = lambda n: f"\ts_waitcnt vmcnt({n})"
    bar = "\ts_barrier"
    assert mod.pre_barrier([q, w(0), ld4, ld4, ld4, w(2), ld4, w(2), w(1), bar, ld4, w(0)]) == 1
    assert mod.pre_barrier([ld4, ld4, ld4, w(2), ld4, w(2), w(0), bar]) == 2              # the fourth load left after the first arrived
    assert mod.pre_barrier([ld4, w(0), ld4, w(0), ld4, ld2, w(0), bar]) == 3
    assert mod.pre_barrier([ld4, ld4, ld4, ld4, w(3), w(0), ld4, ld4, ld2, ld4, w(3), w(1), bar, w(0)]) == 2
    assert mod.pre_barrier([ld4, "\ts_waitcnt lgkmcnt(0)", bar, w(0)]) == 0
