"""GPU: pt_denoise_guided, pt_denoise_guided_demod, pt_select_guided and pt_select_guided_demod (include/pt_guided.h, pt_demod.h, pt_steer.h)
against the float64 reference of tests/_guided_ref64.py, within the per-pixel bound derived there, on the feature records of real scenes with FRAME
and T injected (the inputs of tests/test_guided_ref.py): images narrower than a wave, one pixel wide or high and around the 64 x 4 block of
k_gd_var and k_gd_pass; three scenes at 96x54 with every parameter set; and 577x261 with 8 passes, the smallest image in which the +-256-pixel taps
of the last pass exist on both sides of some pixel in x (and on either side in y) while both image edges cut a block.  The selection may differ
from the reference's only on pixels whose v_K lies within the bound of tol^2, and those stay below 1 % of the image.  Every case also keeps the
share of pixels whose bound says nothing at or below 2 %, and leaves FRAME and T bit for bit as they were."""
import ctypes as C

import numpy as np
import pytest

import _guided_ref64 as ref64
from _reproject_model import frame_in, overlay
from test_guided_ref import CAP, PARAMS, frame_for, moments_for
from test_gpu_guided import CASES

pytestmark = pytest.mark.gpu

# (rel_err, abs_err, max_frames) of the selection that goes with each of CASES
RULES = [(0.05, 0.0, 0), (0.1, 0.0, 0), (0.02, 0.001, 7), (0.3, 0.0, 0), (0.01, 0.0, 5)]
assert len(RULES) == len(CASES) == len(PARAMS) and all(p[:2] == c[1:] for p, c in zip(PARAMS, CASES))
MOUSE = np.array([30.0, 17.0, 0.0], np.float32)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _open(pt, renderer_mod, scene, w, h, mouse=None):
    """(context, feature records, overlay mask)"""
    wl = pt.scenes.build(scene, w, h)
    r = renderer_mod.Renderer(w, h)
    r.load_workload(wl)
    if mouse is not None:
        r.set_buffer(2, mouse)
    ov = overlay(w, h, frame_in(wl.buffers[4], wl.buffers[0], wl.buffers[1], np.asarray(wl.buffers[2] if mouse is None else mouse, np.float32)))
    return r, r.read_features(), ov


def _select_raw(r, rule, floor):
    out = np.zeros((r.H, r.W), np.uint8)
    n = C.c_int64(-1)
    if floor is None:
        assert r._L.pt_select_guided(r._h, C.byref(rule), out.ctypes.data, C.byref(n)) == 0
    else:
        assert r._L.pt_select_guided_demod(r._h, C.byref(rule), floor, out.ctypes.data, C.byref(n)) == 0
    assert set(np.unique(out)) <= {0, 1}
    return out.astype(bool), n.value


def _check(r, feat, ov, fr, T, jobs):
    """jobs: (pass counts, sigmas, min_frames, albedo floor or None, (rel_err, abs_err, max_frames)) each: one reference evaluation.  Returns
    the largest colour deviation as a fraction of the bound, the largest uninformative share, the largest share of near pixels"""
    r.write_frame(fr)
    r.write_moments(T)
    top = [0.0, 0.0, 0.0]
    for ks, sig, mf, floor, (rel, ab, mx) in jobs:
        refs = ref64.filter64(fr, feat, T, tuple(ks), *sig, mf, floor)
        for K in ks:
            ref = refs[K]
            where = (feat.shape[:2], K, sig, mf, floor)
            got = r.denoise_guided(K, *sig, min_frames=mf, albedo_floor=floor)
            assert _bits_equal(r.read_frame(), fr) and _bits_equal(r.read_moments(), T), where
            dev, at = ref64.deviation(got, ref)
            share = ref64.uninformative_share(ref)
            sel, n_sel = _select_raw(r, r.guided_rule(rel, ab, K, *sig, min_frames=mf, max_frames=mx), floor)
            assert _bits_equal(r.read_frame(), fr) and _bits_equal(r.read_moments(), T), where
            act, near, step = ref64.select(ref, T, mf, rel, ab, mx, overlay=ov, demod=floor is not None)
            print(f"  {where}: colour {dev:.4f} of the bound at {at}, uninformative {share:.4f}, near {near.mean():.4f}, selection differs on {int((sel != act).sum())}")
            assert dev <= 1.0, (where, dev, at, got[at], ref["out"][at], ref["bound_c"][at])
            assert share <= CAP, (where, share)
            assert not ((sel != act) & ~near).any(), (where, int(((sel != act) & ~near).sum()), np.argwhere((sel != act) & ~near)[:4].tolist())
            assert near.sum() < 0.01 * sel.size, (where, int(near.sum()))
            assert n_sel == int(sel.sum()), where
            top = [max(a, b) for a, b in zip(top, (dev, share, float(near.mean())))]
    return top


@pytest.mark.parametrize("w,h", [(1, 1), (1, 37), (37, 1), (63, 5), (64, 4), (65, 3), (129, 7)])
def test_edge_shapes(pt, renderer_mod, w, h):
    r, feat, ov = _open(pt, renderer_mod, "C3", w, h)
    fr = frame_for(feat)
    T = moments_for("noisy", fr)
    it, sig, mf = CASES[0]
    top = _check(r, feat, ov, fr, T, [((0, 1, 3, 8), sig, mf, floor, RULES[0]) for floor in (None, PARAMS[0][2])])
    r.close()
    print(f"guided {w}x{h}: largest deviation {top[0]:.4f} of the bound, uninformative {top[1]:.4f}, near {top[2]:.4f}")


@pytest.mark.parametrize("scene", ["C3", "T1", "C6"])
def test_scenes_96x54(pt, renderer_mod, scene):
    r, feat, ov = _open(pt, renderer_mod, scene, 96, 54, MOUSE)
    assert ov.any()
    fr = frame_for(feat)
    T = moments_for("noisy", fr)
    jobs = [((it,), sig, mf, floor, RULES[i]) for i, (it, sig, mf) in enumerate(CASES) for floor in (None, PARAMS[i][2])]
    top = _check(r, feat, ov, fr, T, jobs)
    r.close()
    print(f"guided {scene} 96x54: largest deviation {top[0]:.4f} of the bound, uninformative {top[1]:.4f}, near {top[2]:.4f}")


@pytest.mark.parametrize("demod", [False, True])
@pytest.mark.parametrize("kind", ["noisy", "n8", "converged"])
def test_large_image_8_passes(pt, renderer_mod, kind, demod):
    w, h = 577, 261
    r, feat, ov = _open(pt, renderer_mod, "C3", w, h)
    fr = frame_for(feat)
    T = moments_for(kind, fr)
    it, sig, mf = CASES[4]
    assert it == 8 and 2 * (2 << (it - 1)) < w and 2 * (2 << (it - 1)) < h + 256      # a +-256 tap on both sides in x, on either side in y
    top = _check(r, feat, ov, fr, T, [((it,), sig, mf, PARAMS[4][2] if demod else None, RULES[4])])
    r.close()
    print(f"guided {w}x{h} {kind}{' demodulated' if demod else ''}: largest deviation {top[0]:.4f} of the bound, uninformative {top[1]:.4f}, near {top[2]:.4f}")
