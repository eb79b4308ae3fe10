"""CPU: the generator of scripts/image_fuzz.py held to conditions, so that tests/test_gpu_image_fuzz.py cannot pass on empty work.  Over the suite's
seeds:

  * every plan, translated into a script of tests/c/image_history_check.cpp, gets from the stand-in exactly the answer the plan predicts for
    every history-bound call, code and text (the plan's ledger is pt_image_history.hpp's rules written a second time);
  * every S op is accepted at least twice and every D op appears at least twice; a stale mark, a hold on another image, a camera recorded
    under an older scene and a stale pose are each refused at least once;
  * at least 60 % of every plan's S calls are accepted (the seeds are chosen for that);
  * plan() imports neither torch nor the library, and the same seed gives the same plan."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

from test_image_history import _build, _run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load():
    spec = importlib.util.spec_from_file_location("image_fuzz", os.path.join(ROOT, "scripts", "image_fuzz.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fuzz():
    return load()


@pytest.fixture(scope="module")
def plans(fuzz):
    return {seed: fuzz.plan(seed) for seed in fuzz.SEEDS}


def test_the_suite_has_16_seeds_and_plans_of_10_to_18_state_changing_calls(fuzz, plans):
    assert len(set(fuzz.SEEDS)) == 16
    for seed, p in plans.items():
        s = [c for c in p["calls"] if c["cls"] == "S"]
        assert 10 <= len(s) <= 18, (seed, len(s))
        gaps, run = [], 0
        for c in p["calls"][1:]:
            if c["cls"] == "S":
                gaps.append(run); run = 0
            else:
                run += 1
        assert max(gaps) <= 3, (seed, gaps)
        assert all(c["observed"] for c in s)
    assert {p["workload"] for p in plans.values()} == {"C3", "M5"} and {p["two"] for p in plans.values()} == {False, True}
    d = [c for p in plans.values() for c in p["calls"] if c["cls"] == "D"]
    assert 0.2 < sum(c["observed"] for c in d) / len(d) < 0.45      # about a third


def test_the_stand_in_answers_every_history_bound_call_as_the_plan_predicts(fuzz, plans, tmp_path):
    exe = _build(tmp_path, "check_fuzz", [])
    scripts, maps = {}, {}
    for seed, p in plans.items():
        scripts[f"seed{seed}"], maps[f"seed{seed}"] = fuzz.history_script(p)
    traces = _run(exe, tmp_path, scripts)
    compared = refused = 0
    for name, trace in traces.items():
        p = plans[int(name[4:])]
        answers = [line for line in trace if line.startswith("rc=")]
        assert len(answers) == len(scripts[name]) - 1, name            # one per line after `create`
        for line, k, answer in zip(scripts[name][1:], maps[name][1:], answers):
            if k is None:
                continue
            c = p["calls"][k]
            code = int(answer.split()[0][3:])
            text = answer.split(" error=", 1)[1] if " error=" in answer else ""
            if c["op"] == "refused_upload":
                assert code == c["want"][0] and text.startswith(c["want"][1]), (name, k, answer)
                continue
            want = (0, "") if c["want"] == fuzz.OK else tuple(c["want"])
            assert (code, text) == want, (name, k, c["op"], line, answer, c["want"])
            compared += 1
            refused += code != 0
    assert compared > 300 and refused >= 16, (compared, refused)


def test_every_op_and_the_named_refusals_are_reached(fuzz, plans):
    calls = [c for p in plans.values() for c in p["calls"]]
    accepted = {op: sum(c["op"] == op and c["cls"] == "S" and c["want"] == fuzz.OK for c in calls) for op in fuzz.S_OPS}
    assert {op: n for op, n in accepted.items() if n < 2} == {}
    seen = {op: sum(c["op"] == op and c["cls"] == "D" for c in calls) for op in fuzz.D_OPS}
    assert {op: n for op, n in seen.items() if n < 2} == {}
    assert set(fuzz.REFUSED) <= set(fuzz.D_OPS) and all(c["want"] != fuzz.OK for c in calls if c["op"] in fuzz.REFUSED)
    texts = [c["want"][1] for c in calls if c["cls"] == "S" and c["want"] != fuzz.OK]
    for fragment in ("is no longer the marked one", "the hold belongs to another image", "since the image's camera was recorded",
                     "pt_pose_geometry: the scene was uploaded since pt_pose_create"):
        assert any(fragment in t for t in texts), fragment
    # the pairs the aggregate conditions of the GPU test wait for can occur: a producer, then bloom from its leftover with other calls in between
    far = 0
    for p in plans.values():
        last = None
        for k, c in enumerate(p["calls"]):
            if c["op"] == "filter_for_bloom" or (c["op"] in fuzz.FILTERS and c["observed"]):
                last = k
            elif c["op"] in ("bloom_filtered", "tonemap_bloom") and c["want"] == fuzz.OK:
                assert last is not None
                far += k - last > 1
    assert far >= 2, far
    # ... an observed filter call directly behind another filter or a reprojection, and a despeckle the self-test can swap
    behind = swappable = 0
    for p in plans.values():
        for prev, c in zip(p["calls"], p["calls"][1:]):
            behind += c["cls"] == "D" and c["observed"] and c["op"] in fuzz.FILTERS and prev["op"] != c["op"] and prev["want"] == fuzz.OK and \
                (prev["op"] in fuzz.FILTERS or prev["op"] in fuzz.REPROJECTIONS or prev["op"] == "filter_for_bloom")
        swappable += any(c["op"] == "despeckle" and not c["observed"] for c in p["calls"])
    assert behind >= 3 and swappable >= 5, (behind, swappable)


def test_at_least_60_percent_of_every_plan_s_state_changing_calls_are_accepted(fuzz, plans):
    for seed, p in plans.items():
        assert fuzz.share_accepted(p) >= 0.6, (seed, fuzz.share_accepted(p))


def test_plan_is_pure_and_repeatable(fuzz, plans):
    for seed in fuzz.SEEDS:
        assert json.dumps(fuzz.plan(seed), sort_keys=True) == json.dumps(plans[seed], sort_keys=True), seed
        assert json.loads(json.dumps(plans[seed])) == plans[seed], seed      # a plan written out for --replay is the plan
    probe = ("import importlib.util, sys; spec = importlib.util.spec_from_file_location('image_fuzz', sys.argv[1]); m = importlib.util.module_from_spec(spec); "
             "spec.loader.exec_module(m); [m.plan(s) for s in m.SEEDS]; import ctypes; "
             "bad = [n for n in sys.modules if n == 'torch' or n.startswith('pathtracer') or n == 'ptimport']; "
             "libs = [l for l in open('/proc/self/maps') if 'libpt_hip' in l or 'libamdhip64' in l]; print(bad, len(libs)); sys.exit(1 if bad or libs else 0)")
    r = subprocess.run([sys.executable, "-c", probe, os.path.join(ROOT, "scripts", "image_fuzz.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
