"""-m gpu: k_shade's address-selected state loads against the oracle, bit for bit, at shapes where one wave holds lanes that need a group beside
lanes that read the zero block in its place, and where every path around the loads is taken.

33 x 9 pixels, 3 frames of SAMPLE_RES 8 on a pool of 512 slots: 297 pixels are no multiple of 64 or 256 (the last block has lanes past the end);
891 jobs exceed the pool, so jobs are pulled; a pull comes back empty, so the tail's dense queue is written and read; and lanes end a job
without getting a new one.  96 x 54 with the default pool is the same on several blocks.  One scene per branch of the kernel's template:
3-bit index-stack codes with incLight (G3) and medium (G5) lanes (C3), no transmission (C2), 8-bit codes and the ten floats themselves (nested
shells), texture maps (T1: the instantiations that keep the predicated loads), and directDiffuse."""
import numpy as np
import pytest

from test_gpu_parity import _nested_shells_workload, assert_same, render_both, seeds_for

pytestmark = pytest.mark.gpu

FRAMES = 3
SHAPES = {"small": (33, 9, {"path_slots": 512}), "blocks": (96, 54, {})}


def _workload(pt, scene, W, H):
    if scene == "C3":
        wl = pt.scenes.build("C3", W, H)
    elif scene == "C2":
        wl = pt.scenes.build("C2", W, H)
    elif scene == "shells8":                        # 8 shells: more distinct Ni than 3-bit codes hold -> STK 8
        wl = _nested_shells_workload(pt, W=W, H=H, shells=8)
    elif scene == "shells32":                       # the float-stack variant forced onto the 5-shell scene -> STK 32
        wl = _nested_shells_workload(pt, W=W, H=H, shells=5)
    elif scene == "T1":
        wl = pt.scenes.build("T1", W, H)
    elif scene == "direct":
        return pt.scenes.build("C3", W, H).with_params(RAYTRACING=0, SAMPLE_RES=8)
    return wl.with_params(SAMPLE_RES=8)


@pytest.mark.parametrize("shape", ["small", "blocks"])
@pytest.mark.parametrize("scene", ["C3", "C2", "shells8", "shells32", "T1", "direct"])
def test_state_loads_bit_identical_to_the_oracle(pt, oracle, renderer_mod, scene, shape):
    W, H, opts = SHAPES[shape]
    wl = _workload(pt, scene, W, H)
    if scene == "shells32":
        opts = dict(opts, index_stack_8bit=2)
    # (render_both renders with the counting variants, k_shade<.., STATS>, and again with the shipped ones, and holds the two to the same bits)
    got, ref, cnt, ocnt = render_both(pt, oracle, renderer_mod, wl, FRAMES, **opts)
    assert_same(got, ref, cnt, ocnt)
    assert np.all(got[..., 3] == float(FRAMES))


def test_frame_at_a_time_equals_one_batch(pt, oracle, renderer_mod):
    """the same 891 jobs as one stream of three frames and as three streams of one: job ends that find a new job and job ends that do not fall on
    different segments, the images are the same"""
    W, H, opts = SHAPES["small"]
    wl = _workload(pt, "C3", W, H)
    seeds = seeds_for(pt, 1, FRAMES)
    r = renderer_mod.Renderer(W, H)
    for k, v in opts.items():
        r.set_option(k, v)
    r.load_workload(wl)
    r.reset_frame()
    r.render_batch(1, seeds)
    batch = r.read_frame().copy()
    r.reset_frame()
    for k, s in enumerate(seeds):
        r.render(1 + k, s)
    single = r.read_frame().copy()
    r.close()
    assert np.array_equal(batch, single, equal_nan=True)
    ref, _ = oracle.render_frames(oracle.Scene.from_workload(wl), W, H, 1, FRAMES, seeds, nthreads=8)
    assert_same(batch, ref)
