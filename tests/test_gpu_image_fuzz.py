"""GPU: random sequences of the image-space and geometry calls (scripts/image_fuzz.py) on one warm context against a cold, serial twin: the
record caches, the mark, the hold and the camera records, the scratch the filters, the reprojections and the poses share, and the order of the
calls against a running frame stream, in orders nobody chose.  tests/test_image_fuzz_plan.py holds the generator to its conditions on the CPU;
here every seed's run must agree call by call, the seeds together must have done the work the aggregate conditions name, and the comparison
must notice a distractor that stores."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _load():
    spec = importlib.util.spec_from_file_location("image_fuzz", os.path.join(ROOT, "scripts", "image_fuzz.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FUZZ = _load()


@pytest.fixture(scope="module")
def state():
    """what the seeds leave behind: the counts of the aggregate conditions, and whether a call faulted"""
    return dict(fault=None, counts={}, ran=[])


def _run(state, pt, renderer_mod, seed, counts):
    assert state["fault"] is None, f"not run: {state['fault']}"      # after a fault nothing more touches a context
    try:
        FUZZ.run(FUZZ.plan(seed), (renderer_mod, pt.scenes), counts)
    except FUZZ.DeviceFault as e:
        state["fault"] = f"seed {seed}: {e}"
        raise


@pytest.mark.parametrize("seed", FUZZ.SEEDS)
def test_random_sequences(state, pt, renderer_mod, seed):
    counts = {}
    _run(state, pt, renderer_mod, seed, counts)
    state["ran"].append(seed)
    total = state["counts"]
    for op, n in counts.get("accepted", {}).items():
        total.setdefault("accepted", {})[op] = total.get("accepted", {}).get(op, 0) + n
    for key in ("partly_kept", "changed", "refusals"):
        total.setdefault(key, set()).update(counts.get(key, ()))
    total["filter_after_another"] = total.get("filter_after_another", 0) + counts.get("filter_after_another", 0)
    print(f"seed {seed}: accepted {counts.get('accepted')}, refusals {sorted(counts.get('refusals', ()))}")


def test_the_checker_notices_a_storing_distractor(state, pt, renderer_mod, monkeypatch):
    """self-test: with one unobserved despeckle of the warm context turned into despeckle_frame, the comparison fails for some seed no later than
    at the first S call behind the swapped one (an observed D call in between may see the changed FRAME first), and never before the swap.
    (A swapped call that clamps no pixel still writes the image's camera, which only a later mark or hold can tell: such a seed may fail later.)"""
    monkeypatch.setenv("IMAGE_FUZZ_SELFTEST", "1")
    at_once = later = 0
    for seed in FUZZ.SEEDS:
        assert state["fault"] is None, f"not run: {state['fault']}"
        p, counts = FUZZ.plan(seed), {}
        try:
            FUZZ.run(p, (renderer_mod, pt.scenes), counts)
        except FUZZ.Mismatch as e:
            at = counts["swapped"]
            nxt = next(k for k in range(at + 1, len(p["calls"])) if p["calls"][k]["cls"] == "S")
            assert e.at > at, (seed, at, str(e))
            print(f"seed {seed}: swapped call {at}, next S call {nxt}, noticed: {e}")
            at_once += e.at <= nxt
            later += e.at > nxt
        except FUZZ.DeviceFault as e:                                # (a camera record the twin does not have can turn a later answer: also noticed)
            assert "HIP error" not in str(e) and "swapped" in counts, (seed, str(e))
            later += 1
    assert at_once >= 1, (at_once, later)


def test_the_seeds_together_did_the_work(state):
    """the last test of the module: what the seeds above left in `state`"""
    assert state["fault"] is None and sorted(state["ran"]) == sorted(FUZZ.SEEDS), (state["fault"], state["ran"])
    total = state["counts"]
    print(total)
    assert total["partly_kept"] == set(FUZZ.REPROJECTIONS), total["partly_kept"]      # each form kept 0 < kept < W * H at least once
    assert total["changed"] == {"history_merge", "despeckle_frame"}, total["changed"]
    assert total["filter_after_another"] >= 1
