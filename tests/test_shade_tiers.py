"""The shading kernel's chain of dependent loads, read statically from the compiled code (scripts/shade_tiers.py; hipcc, no GPU).

k_shade is latency bound: each vmcnt-separated load tier is a round trip of about 1100 cycles beside the intersect kernel.  An edit that
serialises a load behind another's wait, or that spills to scratch, shows here before it shows in a benchmark."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3 = "k_shade<3,false,false,false,false>"           # the variant bench.py's default workload runs
C3_MAX_TIERS = 16                                   # the count in layout order: an upper bound on what one wave waits out in sequence


def _report():
    spec = importlib.util.spec_from_file_location("shade_tiers", os.path.join(ROOT, "scripts", "shade_tiers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        return mod.report(open(mod.compile_asm(d)).read())


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_c3_shading_kernel_tiers_and_scratch():
    r = _report()
    assert len(r) == 28, sorted(r)                  # every instantiation was found
    v = r[C3]
    assert v["scratch_bytes"] == 0, v
    assert v["tiers"] <= C3_MAX_TIERS, v
    assert v["waves_per_simd"] >= 6, v
