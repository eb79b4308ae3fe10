"""CPU, files only: what libpt_hip.so is made of is one list (build.HIP_UNITS), and build.kernel_source_hash() covers the text of the render
kernels and nothing of the host side (build.KERNEL_HASH_FILES), so that the hash the committed counter summaries carry moves with the kernels alone."""
import os
import re

import ptimport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "pathtracer-0_amd", "csrc", "hip")


def _build():
    ptimport.load()
    from pathtracer_0_amd import build
    return build


def _text(name):
    with open(os.path.join(HIP, name), encoding="utf-8") as f:
        return f.read()


def _render_unit_files():
    """pt_hip.hip and what it includes with #include "...", transitively, as far as it lies in csrc/hip"""
    seen, todo = set(), ["pt_hip.hip"]
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.add(name)
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', _text(name), re.M):
            path = os.path.normpath(os.path.join(HIP, inc))
            if os.path.dirname(path) == HIP and os.path.exists(path):
                todo.append(os.path.basename(path))
    return sorted(seen)


def test_every_hip_file_is_a_unit_of_the_library():
    build = _build()
    on_disk = sorted(f for f in os.listdir(HIP) if f.endswith(".hip"))
    assert sorted(build.HIP_UNITS) == on_disk
    assert build.HIP_UNITS[0] == "pt_hip.hip" and len(set(build.HIP_UNITS)) == len(build.HIP_UNITS)
    for f in build.HIP_UNITS + build.KERNEL_HASH_FILES:
        assert os.path.isfile(os.path.join(HIP, f)), f


def test_the_hash_covers_every_file_with_render_kernel_text():
    build = _build()
    files = _render_unit_files()
    assert "pt_kernels.hpp" in files and "pt_context.hpp" in files and "pt_stream_dev.hpp" in files      # the walk follows the includes
    with_kernels = [f for f in files if "__global__" in _text(f)]
    assert with_kernels, "the walk found no kernel at all"
    for f in with_kernels:
        assert f in build.KERNEL_HASH_FILES, f + " holds a __global__ kernel of the render path and is not hashed"


def test_the_hashed_files_hold_no_host_code():
    build = _build()
    for f in build.KERNEL_HASH_FILES:
        text = _text(f)
        for word in ("pt_ctx", "hipLaunchKernelGGL", "hipStream", "HIP_TRY"):
            assert word not in text, f + " is hashed as kernel text and mentions " + word


def test_build_variant_takes_the_units_from_build():
    with open(os.path.join(ROOT, "scripts", "build_variant.py"), encoding="utf-8") as f:
        text = f.read()
    assert not re.findall(r"\w+\.hip\b", text), "scripts/build_variant.py names .hip files of its own"
    assert "build.HIP_UNITS" in text
