"""GPU: adaptive sampling steered by the guided filter (include/pt_steer.h).

pt_render_mask renders only the reference's own jobs, so FRAME and T are checked bit for bit against tests/_adaptive_model.py's Model fed with the
oracle's one-frame images.  pt_select_guided is checked against the float32 model of tests/_steer_model.py on the feature records of real scenes,
with FRAME and T injected: steps 1-4 exactly, step 5 up to the filter's known ~1e-4 disagreement.  pt_render_adaptive_guided must equal the two
calls made one after the other, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from _adaptive_model import Model
from _reproject_model import frame_in, overlay
from _steer_model import select_guided as model
from conftest import frames_equal
from test_gpu_guided import _inject
from test_gpu_parity import _no_vn_workload
from test_gpu_reproject import move

pytestmark = pytest.mark.gpu

W, H = 128, 72
NF = 10
MOUSE = np.array([40.0, 30.0, 0.0], np.float32)        # the overlay: pixel (40, 30) (resolution 128: |d| < 0.64)


def _seeds(pt, first, n):
    return [pt.scenes.frame_seed(f) for f in range(first, first + n)]


def _cols(pt, oracle, wl, w=W, h=H):
    sc = oracle.Scene.from_workload(wl)
    return [oracle.render(sc, w, h, 1, pt.scenes.frame_seed(f), nthreads=8)[0][..., :3].copy() for f in range(1, NF + 1)]


@pytest.fixture(scope="module")
def c3(pt, oracle):
    wl = pt.scenes.build("C3", W, H)
    return wl, _cols(pt, oracle, wl)


@pytest.fixture(scope="module")
def novn(pt, oracle):
    wl = _no_vn_workload(pt, W, H)
    return wl, _cols(pt, oracle, wl)


def _open(renderer_mod, wl, w=W, h=H, **kw):
    r = renderer_mod.Renderer(w, h, **kw)
    r.load_workload(wl)
    r.reset_frame()
    return r


def _overlay(wl, w=W, h=H, mouse=MOUSE):
    return overlay(w, h, frame_in(wl.buffers[4], wl.buffers[0], wl.buffers[1], mouse))


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _masks(ov):
    """(first, n, mask) of successive pt_render_mask calls: frame 1 first (it overwrites FRAME), a random mask, a block with the overlay
    inside it, a checkerboard, everything"""
    rs = np.random.RandomState(11)
    rand = rs.rand(H, W) < 0.3
    block = np.zeros((H, W), bool)
    block[20:50, 25:70] = True
    assert (block & ov).any()
    yy, xx = np.mgrid[0:H, 0:W]
    checker = ((yy // 8 + xx // 8) % 2) == 0
    return [(1, 2, rand | block), (3, 2, rand), (5, 1, block), (6, 3, checker), (9, 2, np.ones((H, W), bool))]


# ---------------------------------------------------------------------------------------------------------------- pt_render_mask

@pytest.mark.parametrize("scene", ["c3", "novn"])
def test_render_mask_equals_the_model(pt, renderer_mod, request, scene):
    wl, cols = request.getfixturevalue(scene)
    ov = _overlay(wl)
    assert ov.any()
    r = _open(renderer_mod, wl)
    r.set_buffer(2, MOUSE)
    m = Model(cols)
    for first, n, mask in _masks(ov):
        got = r.render_mask(first, _seeds(pt, first, n), mask.astype(np.uint8) * 7)      # any non-zero byte selects
        act = mask & ~ov
        m.frames(first, n, act)
        assert got == int(act.sum())
        assert frames_equal(r.read_frame(), m.F), (first, int((~((r.read_frame() == m.F) | np.isnan(m.F))).sum()))
        assert frames_equal(r.read_moments(), m.T)                    # (NaN == NaN: the no-vn scene's sums)
    assert (r.read_frame()[ov] == 0).all()
    if scene == "novn":
        assert np.isnan(m.F[..., :3]).any()
    r.close()


def test_render_mask_on_every_context(pt, renderer_mod, c3):
    wl, cols = c3
    ov = _overlay(wl)
    outs = []
    for kw in ({}, {"devices": [0, 0]}):
        r = _open(renderer_mod, wl, **kw)
        r.set_buffer(2, MOUSE)
        counts = [r.render_mask(first, _seeds(pt, first, n), mask) for first, n, mask in _masks(ov)[:4]]
        outs.append((counts, r.read_frame(), r.read_moments()))
        r.close()
    assert outs[0][0] == outs[1][0] and frames_equal(outs[0][1], outs[1][1]) and _bits_equal(outs[0][2], outs[1][2])
    # two shard contexts of pt_create: each takes its own pixels from the full mask
    F = np.zeros((H, W, 4), np.float32)
    total = [0] * 4
    for rank in (0, 1):
        own = np.zeros(W * H, bool)
        sm = renderer_mod.shard_map(W, H, rank, 2)
        own[sm[sm >= 0]] = True
        own = own.reshape(H, W)
        r = _open(renderer_mod, wl, shard_rank=rank, shard_count=2)
        r.set_buffer(2, MOUSE)
        for i, (first, n, mask) in enumerate(_masks(ov)[:4]):
            got = r.render_mask(first, _seeds(pt, first, n), mask)
            assert got == int((mask & ~ov & own).sum())
            total[i] += got
        F[own] = r.read_frame()[own]
        r.close()
    assert total == outs[0][0] and frames_equal(F, outs[0][1])


# ---------------------------------------------------------------------------------------------------------------- pt_select_guided

SW, SH = 96, 54                                         # tests/test_gpu_guided.py's injected image
SMOUSE = np.array([30.0, 17.0, 0.0], np.float32)
INF = float("inf")
# (iterations, sigmas, min_frames, rel_err, abs_err, max_frames)
RULES = [(5, (2.0, 0.3, 0.05, 0.1), 4, 0.05, 0.0, 0), (0, (2.0, 0.3, 0.05, 0.1), 4, 0.1, 0.0, 0), (3, (1.0, INF, 0.1, INF), 2, 0.02, 0.001, 7),
         (2, (INF, 0.3, 0.05, 0.1), 4, 0.3, 0.0, 0), (8, (10.0, 0.2, 0.02, 0.05), 6, 0.01, 0.0, 5)]


def _check_select(got, n_got, want, d):
    step = d["step"]
    exact = step <= 4
    assert np.array_equal(got[exact], want[exact]), int((got[exact] != want[exact]).sum())
    v, t2 = d["v"].astype(np.float64), d["tol2"].astype(np.float64)
    with np.errstate(all="ignore"):                                     # (a v_K of +inf is active on both sides: no margin)
        near = np.isfinite(v) & np.isfinite(t2) & (np.abs(v - t2) <= 1e-3 * np.maximum(np.abs(v), np.abs(t2)))
    bad = (step == 5) & (got != want)
    assert not (bad & ~near).any(), int((bad & ~near).sum())
    assert ((step == 5) & near).sum() < 0.01 * got.size
    assert n_got == int(got.sum())


def _select_raw(r, rule):
    out = np.zeros((r.H, r.W), np.uint8)
    n = C.c_int64(-1)
    assert r._L.pt_select_guided(r._h, C.byref(rule), out.ctypes.data, C.byref(n)) == 0
    assert set(np.unique(out)) <= {0, 1}
    return out.astype(bool), n.value


@pytest.mark.parametrize("scene", ["C3", "T1", "C6"])
def test_select_matches_the_model(pt, renderer_mod, scene):
    wl = pt.scenes.build(scene, SW, SH)
    r = renderer_mod.Renderer(SW, SH)
    r.load_workload(wl)
    r.set_buffer(2, SMOUSE)
    ov = _overlay(wl, SW, SH, SMOUSE)
    assert ov.any()
    feat = r.read_features()
    fr, T = _inject(feat)
    # the injected T leaves many pixels below min_frames without a pooled estimate (v = +inf, spread by the passes); the second one has
    # n >= 8 and no NaN sum, so that step 5 compares finite variances everywhere
    T2 = T.copy()
    T2[..., 2] = np.maximum(T2[..., 2], 8.0)
    T2[40, 50, :2] = (4.0, 3.0)
    steps = set()
    for moments, rules in ((T, RULES), (T2, [rule[:5] + (0,) for rule in RULES])):
        r.write_frame(fr)
        r.write_moments(moments)
        for it, sig, mf, rel, ab, mx in rules:
            got, n = _select_raw(r, r.guided_rule(rel, ab, it, *sig, min_frames=mf, max_frames=mx))
            want, d = model(fr, feat, moments, it, *sig, mf, rel, ab, mx, overlay=ov, detail=True)
            _check_select(got, n, want, d)
            assert np.array_equal(r.select_guided(rel, ab, it, *sig, min_frames=mf, max_frames=mx), got)
            steps |= set(np.unique(d["step"]).tolist())
        assert _bits_equal(r.read_frame(), fr) and _bits_equal(r.read_moments(), moments)      # neither is modified
    assert steps == {1, 2, 3, 4, 5}                                     # every step decided some pixel
    r.close()


def test_select_without_moments_is_everything_but_the_overlay(pt, renderer_mod):
    wl = pt.scenes.build("C3", SW, SH)
    r = renderer_mod.Renderer(SW, SH)
    r.load_workload(wl)
    r.set_buffer(2, SMOUSE)
    r.render_batch(1, _seeds(pt, 1, 2))                 # T never allocated: read as zeros, n = 0 < min_frames
    got, n = _select_raw(r, r.guided_rule(0.05))
    ov = _overlay(wl, SW, SH, SMOUSE)
    assert np.array_equal(got, ~ov) and n == SW * SH - int(ov.sum())
    assert not r.read_moments().any()
    with pytest.raises(renderer_mod.PtError):           # ... and still none: pt_denoise_guided needs moments
        r.denoise_guided()
    r.close()


# ---------------------------------------------------------------------------------------------------------------- pt_render_adaptive_guided

# (first, n, rel_err, min_frames, max_frames) of successive calls
GCALLS = [(1, 2, 0.05, 2, 0), (3, 2, 0.05, 2, 0), (5, 2, 0.05, 4, 0), (7, 2, 0.02, 4, 9), (9, 2, 0.05, 4, 0)]


def _guided_run(pt, renderer_mod, wl, split, **kw):
    r = _open(renderer_mod, wl, **kw)
    r.set_buffer(2, MOUSE)
    counts = []
    for first, n, rel, mf, mx in GCALLS:
        if split:
            mask = r.select_guided(rel, min_frames=mf, max_frames=mx)
            counts.append(r.render_mask(first, _seeds(pt, first, n), mask))
        else:
            counts.append(r.render_adaptive_guided(first, _seeds(pt, first, n), rel, min_frames=mf, max_frames=mx))
    out = (counts, r.read_frame(), r.read_moments())
    r.close()
    return out


def test_render_adaptive_guided_is_select_then_mask(pt, renderer_mod, c3):
    wl, _ = c3
    runs = {(split, multi): _guided_run(pt, renderer_mod, wl, split, **({"devices": [0, 0]} if multi else {}))
            for split in (False, True) for multi in (False, True)}
    base = runs[(False, False)]
    assert base[0][0] == W * H - int(_overlay(wl).sum())               # no moments yet: everything but the overlay
    assert any(0 < c < base[0][0] for c in base[0][1:]), base[0]         # a real selection afterwards
    for key, (counts, F, T) in runs.items():
        assert counts == base[0], key
        assert frames_equal(F, base[1]) and _bits_equal(T, base[2]), key


def test_frozen_pixels_resume(pt, renderer_mod, c3):
    """four frames on every pixel, then the guided rule: some pixel with four identical frames (own variance 0, inactive under pt_adaptive.h's
    rule however small its tolerance) is active, and the next call renders it"""
    wl, cols = c3
    m = Model(cols)
    r = _open(renderer_mod, wl)
    ones = np.ones((H, W), bool)
    assert r.render_mask(1, _seeds(pt, 1, 4), ones) == W * H
    m.frames(1, 4, ones)
    T = r.read_moments()
    assert frames_equal(T, m.T)
    own_zero = (T[..., 1] - T[..., 0] * (T[..., 0] / T[..., 2]) == 0) & (T[..., 2] >= 4)
    act = r.select_guided(0.05)
    resumed = act & own_zero
    assert resumed.sum() >= 10, int(resumed.sum())
    before = r.read_frame()[..., 3]
    n = r.render_adaptive_guided(5, _seeds(pt, 5, 2), 0.05)
    after = r.read_frame()[..., 3]
    r.close()
    assert n == int(act.sum())
    assert (after[resumed] == before[resumed] + 2).all()


def test_disoccluded_pixels_are_active_after_reprojection(pt, renderer_mod, c3):
    wl, _ = c3
    r = _open(renderer_mod, wl)
    r.set_buffer(2, MOUSE)
    r.render_adaptive_guided(1, _seeds(pt, 1, 4), 0.05)
    A = (wl.buffers[0], wl.buffers[1])
    B = move(*A, forward=0.04, strafe=0.03, yaw=0.03)
    r.set_buffer(0, np.asarray(B[0], np.float32))
    r.set_buffer(1, np.asarray(B[1], np.float32))
    kept = r.reproject_frame()
    F = r.read_frame()
    ov = overlay(W, H, frame_in(wl.buffers[4], B[0], B[1], MOUSE))
    fresh = (F[..., 3] == 0) & ~ov
    assert 0 < kept < W * H and fresh.any()
    act = r.select_guided(0.05)
    assert act[fresh].all() and not act[ov].any()
    n = r.render_adaptive_guided(5, _seeds(pt, 5, 1), 0.05)
    assert n == int(act.sum())
    assert (r.read_frame()[..., 3][fresh] == 1).all()
    r.close()


# ---------------------------------------------------------------------------------------------------------------- errors

def test_errors_and_unsupported_contexts(pt, renderer_mod, c3):
    from pathtracer_0_amd.renderer import GuidedRule, PtError
    wl, _ = c3
    r = _open(renderer_mod, wl)
    r.render_adaptive_guided(1, _seeds(pt, 1, 2), 0.05)
    F, T = r.read_frame(), r.read_moments()
    L, h = r._L, r._h
    seeds = np.array(_seeds(pt, 3, 2), np.int32).ctypes.data
    mask = np.ones((H, W), np.uint8)
    out = np.zeros((H, W), np.uint8)
    n = C.c_int64(-1)
    good = r.guided_rule(0.05)
    bad = []
    for field, v in (("iterations", -1), ("iterations", 9), ("sigma_lum", 0.0), ("sigma_normal", -1.0), ("sigma_depth", float("nan")),
                     ("sigma_albedo", 0.0), ("min_frames", 1), ("rel_err", -0.1), ("rel_err", float("nan")), ("abs_err", -1.0),
                     ("abs_err", float("nan")), ("max_frames", -1)):
        b = GuidedRule.from_buffer_copy(good)
        setattr(b, field, v)
        bad.append(b)
    for b in bad:
        assert L.pt_select_guided(h, C.byref(b), out.ctypes.data, C.byref(n)) == -1 and n.value == 0
        assert L.pt_render_adaptive_guided(h, 3, 2, seeds, C.byref(b), C.byref(n)) == -1 and n.value == 0
    assert L.pt_select_guided(None, C.byref(good), out.ctypes.data, None) == -1
    assert L.pt_select_guided(h, None, out.ctypes.data, None) == -1
    assert L.pt_select_guided(h, C.byref(good), None, None) == -1
    assert L.pt_render_adaptive_guided(None, 3, 2, seeds, C.byref(good), None) == -1
    assert L.pt_render_adaptive_guided(h, 3, 2, None, C.byref(good), None) == -1
    assert L.pt_render_adaptive_guided(h, 3, 2, seeds, None, None) == -1
    assert L.pt_render_adaptive_guided(h, 3, 0, seeds, C.byref(good), None) == -1
    assert L.pt_render_mask(None, 3, 2, seeds, mask.ctypes.data, None) == -1
    assert L.pt_render_mask(h, 3, 2, None, mask.ctypes.data, None) == -1
    assert L.pt_render_mask(h, 3, 2, seeds, None, None) == -1
    assert L.pt_render_mask(h, 3, 0, seeds, mask.ctypes.data, C.byref(n)) == -1 and n.value == 0
    p = np.array(wl.buffers[4], np.float32).copy()
    p[10] = 1.0                                        # Parameters.DEBUG
    r.set_buffer(4, p)
    for call in (lambda: r.render_mask(3, _seeds(pt, 3, 2), mask), lambda: r.render_adaptive_guided(3, _seeds(pt, 3, 2), 0.05)):
        with pytest.raises(PtError) as e:
            call()
        assert e.value.code == -5
    r.set_buffer(4, wl.buffers[4])
    assert frames_equal(r.read_frame(), F) and _bits_equal(r.read_moments(), T)      # no failed call touched FRAME or T
    r.close()
    g = _open(renderer_mod, wl, devices=[0, 0])
    g.set_buffer(4, p)
    with pytest.raises(PtError) as e:
        g.render_adaptive_guided(1, _seeds(pt, 1, 2), 0.05)
    assert e.value.code == -5
    g.close()
    for kw in (dict(shard_rank=0, shard_count=2), dict(devices=[0], first_shard=0, total_shards=2)):
        q = _open(renderer_mod, wl, **kw)
        assert q.render_mask(1, _seeds(pt, 1, 2), mask) > 0               # rendering a mask works on every context
        Fq = q.read_frame()
        for call in (lambda: q.select_guided(0.05), lambda: q.render_adaptive_guided(3, _seeds(pt, 3, 2), 0.05)):
            with pytest.raises(PtError) as e:
                call()
            assert e.value.code == -5, kw
        assert frames_equal(q.read_frame(), Fq)
        q.close()
