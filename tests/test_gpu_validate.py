"""GPU: history validation (pt_history_hold, pt_history_merge; include/pt_validate.h) against the float32 model of tests/_validate_model.py, bit
for bit in FRAME, T, kappa and the count: the whole move - reproject - hold - render - merge path on M2, an emitter edit, injected values, an
interleaved render, contexts, later renders and every error."""
import ctypes as C

import numpy as np
import pytest

import _validate_model as VM
from _reproject_model import frame_in
from conftest import frames_equal

pytestmark = pytest.mark.gpu

W, H = 96, 54
GEOMETRY = (3, 7, 10, 11, 12, 13)
NO_MOUSE = np.array([-1.0e6, -1.0e6, 0.0], np.float32)
LIGHT_KE = slice(48 * 3 + 17, 48 * 3 + 20)                      # Ke of _cornell_materials' fourth material in binding 14


def _seeds(pt, first, n):
    return [pt.scenes.frame_seed(f) for f in range(first, first + n)]


def _fin(wl, mouse=NO_MOUSE):
    return frame_in(wl.buffers[4], wl.buffers[0], wl.buffers[1], mouse)


def _differ(a, b):
    return int((np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)).reshape(a.shape[0], a.shape[1], -1).any(-1).sum())


def _merge_against_model(r, wl, Hh, V, rule, mouse=NO_MOUSE, tag=None):
    """reads N, U and the records, merges on the device with kappa asked for, and holds the four results to the model"""
    N, U, feat = r.read_frame(), r.read_moments(), r.read_features()
    n, kappa = r.history_merge(r.validate_rule(*rule), want_kappa=True)
    F, T = r.read_frame(), r.read_moments()
    wF, wT, wk, wn = VM.merge(N, U, Hh, V, feat, _fin(wl, mouse), *rule)
    assert frames_equal(kappa, wk), (tag, "kappa", _differ(kappa[..., None], wk[..., None]))
    assert frames_equal(F, wF), (tag, "FRAME", _differ(F, wF))
    assert frames_equal(T, wT), (tag, "T", _differ(T, wT))
    assert n == wn, (tag, n, wn)
    return N, U, F, T, kappa, n


def _m2_held(pt, renderer_mod, w=W, h=H, mouse=NO_MOUSE, **kw):
    """8 frames of M2 at step 0, the light slid to step 10, the image reprojected across the move and held: the context, the new workload, H and V"""
    wl0, wl1 = pt.scenes.m2_relit(0, w, h), pt.scenes.m2_relit(10, w, h)
    r = renderer_mod.Renderer(w, h, **kw)
    r.load_workload(wl0)
    r.record_moments(True)
    r.render_batch(1, _seeds(pt, 1, 8))
    r.motion_mark()
    for b in GEOMETRY:
        r.set_buffer(b, wl1.buffers[b])
    r.set_buffer(2, mouse)
    r.reproject_frame_moved()
    Hh, V = r.read_frame(), r.read_moments()
    r.history_hold()
    return r, wl1, Hh, V


@pytest.mark.parametrize("w,h,radius,mouse", [(96, 54, 3, (30.0, 17.0)), (96, 54, 1, None), (96, 54, 4, None),
                                              (130, 35, 3, None), (130, 35, 4, None),          # 3 x 3 blocks, both edges partial
                                              (100, 7, 1, None), (100, 7, 3, None), (100, 7, 4, None),      # lower than the window
                                              (5, 3, 1, None), (5, 3, 3, None), (5, 3, 4, None)])
def test_the_full_path_on_m2_matches_the_model(pt, renderer_mod, w, h, radius, mouse):
    mouse = NO_MOUSE if mouse is None else np.array([mouse[0], mouse[1], 0.0], np.float32)
    r, wl, Hh, V = _m2_held(pt, renderer_mod, w, h, mouse)
    assert (Hh[..., 3] > 0).any() and (V[..., 2] > 0).any()
    assert not r.read_frame().any() and not r.read_moments().any()      # the hold emptied the image ...
    r.render_batch(9, _seeds(pt, 9, 4))
    rule = (radius, 3.0, 5.0, 0.9)
    N, U, F, T, kappa, n = _merge_against_model(r, wl, Hh, V, rule, mouse, (w, h, radius))      # ... and left its camera: the merge is accepted
    print(f"M2 {w}x{h} radius {radius}: {n} pixels reduced, kappa mean {kappa.mean():.3f}, min {kappa.min():.3f}")
    if w * h >= 96 * 54:
        assert 0 < n < w * h and (kappa == 1).any() and ((kappa > 0) & (kappa < 1)).any()
    if mouse is not NO_MOUSE:
        under = VM.overlay(w, h, _fin(wl, mouse))
        assert under.any() and (kappa[under] == 1).all() and frames_equal(F[under], Hh[under])      # nothing is rendered there: 0 + H
    r.close()


def test_an_emitter_edit_is_carried_without_a_reprojection(pt, renderer_mod):
    """Ke of the light through binding 14, which both reprojections refuse: render, dim the light, hold, render, merge"""
    wl = pt.scenes.m2_relit(0, W, H)
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl)
    r.record_moments(True)
    r.render_batch(1, _seeds(pt, 1, 8))
    Hh, V = r.read_frame(), r.read_moments()
    mtl = wl.buffers[14].copy()
    assert (mtl[LIGHT_KE] == 15.0).all()
    mtl[LIGHT_KE] = 3.0
    r.set_buffer(14, mtl)
    with pytest.raises(renderer_mod.PtError):
        r.reproject_frame()
    r.history_hold()
    r.render_batch(9, _seeds(pt, 9, 4))
    N, U, F, T, kappa, n = _merge_against_model(r, wl, Hh, V, (3, 3.0, 5.0, 0.9))
    print(f"Ke 15 -> 3: {n} of {W * H} pixels reduced, kappa mean {kappa.mean():.3f}")
    assert n > W * H // 4                                               # the whole room is lit by this light
    r.close()


def _injected(seed):
    """N, U, H, V with every value the rule has a branch for"""
    rs = np.random.RandomState(seed)

    def pair(mean, n):
        cnt = np.full((H, W), n, np.float32)
        Y = (mean + 0.1 * rs.randn(int(n), H, W)).astype(np.float32)
        fr = np.stack([Y.sum(0) * c for c in (1.0, 0.5, 0.25)] + [cnt], -1).astype(np.float32)
        T = np.stack([Y.sum(0), (Y * Y).sum(0), cnt, np.zeros((H, W), np.float32)], -1).astype(np.float32)
        return fr, T
    Hh, V = pair(0.4, 16)
    N, U = pair(0.4, 4)
    Nb, Ub = pair(0.8, 4)
    N[:, 40:], U[:, 40:] = Nb[:, 40:], Ub[:, 40:]                      # the light changed on the right
    inf, nan = np.inf, np.nan
    U[3, 5, 0], U[3, 9, 1], V[3, 13, 0], V[3, 17, 1] = nan, inf, -inf, nan          # a sum that is not finite unpairs the tap
    U[8, 50, 0], V[8, 60, 1] = inf, nan
    U[12, 5:9, 2], U[12, 50:54, 2] = 0.0, 0.0                           # n = 0, 0.5 and negative, on either side
    U[14, 5:9, 2], V[14, 50:54, 2] = 0.5, 0.5
    U[16, 5:9, 2], V[16, 50:54, 2] = -3.0, -1.0
    Hh[20, 5:9, 3], Hh[20, 50:54, 3] = 0.0, 0.0                         # H.a = 0 with V.n > 0: merged, not counted
    Hh[22, 50, 0], Hh[22, 6, 1], Hh[23, 52, 3] = inf, nan, inf          # an inf in H under kappa = 0 and a NaN under kappa = 1
    N[24, 7, 2], N[24, 55, 0] = nan, -inf
    U[30:36, 60:70, :2] = 3.0e38                                        # sums that overflow float32 within a window
    V[30:36, 20:30, 1] = 3.0e38
    U[40:44, 70:80, 2] = inf                                            # an infinite count is >= 1
    return N, U, Hh, V


@pytest.mark.parametrize("radius,z", [(3, (3.0, 5.0)), (4, (0.0, 40.0)), (1, (2.0, 4.0))])
def test_injected_values_match_the_model(pt, renderer_mod, radius, z):
    wl = pt.scenes.build("C3", W, H)
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl)
    r.record_moments(True)
    N, U, Hh, V = _injected(7)
    r.write_frame(Hh)
    r.write_moments(V)
    r.history_hold()
    r.write_frame(N)
    r.write_moments(U)
    _, _, F, T, kappa, n = _merge_against_model(r, wl, Hh, V, (radius, z[0], z[1], 0.9), tag=(radius, z))
    assert 0 < n < W * H and (kappa == 0).any() and (kappa == 1).any() and ((kappa > 0) & (kappa < 1)).any()
    r.close()


def test_unrendered_pixels_take_their_neighbours_kappa(pt, renderer_mod):
    """behind pt_render_interleaved, stride 2: three pixels of four hold nothing new, and still lose the history their rendered neighbours contradict"""
    r, wl, Hh, V = _m2_held(pt, renderer_mod)
    assert r.render_interleaved(9, _seeds(pt, 9, 4), stride=2) == (W // 2) * (H // 2)
    N, U, F, T, kappa, n = _merge_against_model(r, wl, Hh, V, (3, 3.0, 5.0, 0.9))
    empty = (U[..., 2] == 0) & (N[..., 3] == 0)
    assert int(empty.sum()) == W * H - (W // 2) * (H // 2)
    assert (empty & (kappa < 1) & (Hh[..., 3] > 0)).any()
    r.close()


def test_nothing_rendered_gives_the_held_image_back(pt, renderer_mod):
    r, wl, Hh, V = _m2_held(pt, renderer_mod)
    n, kappa = r.history_merge(want_kappa=True)
    assert n == 0 and (kappa == 1).all()
    assert frames_equal(r.read_frame(), Hh) and frames_equal(r.read_moments(), V)
    r.close()


def _sequence(pt, renderer_mod, **kw):
    r, wl, Hh, V = _m2_held(pt, renderer_mod, **kw)
    empty = (r.read_frame(), r.read_moments())
    r.render_batch(9, _seeds(pt, 9, 4))
    n, kappa = r.history_merge(want_kappa=True)
    mid, midT = r.read_frame(), r.read_moments()
    r.render_batch(13, _seeds(pt, 13, 2))
    out, outT = r.read_frame(), r.read_moments()
    r.close()
    return wl, Hh, V, empty, n, kappa, mid, midT, out, outT


def test_multi_stream_context_equals_one_stream(pt, renderer_mod):
    one = _sequence(pt, renderer_mod)
    assert 0 < one[4] < W * H
    for kw in ({"devices": [0, 0]}, {"devices": [0]}):
        got = _sequence(pt, renderer_mod, **kw)
        assert not got[3][0].any() and not got[3][1].any(), kw
        assert got[4] == one[4], kw
        for a, b in zip(got[1:3] + got[5:], one[1:3] + one[5:]):
            assert frames_equal(a, b), kw


def test_later_renders_equal_renders_on_the_written_result(pt, renderer_mod):
    wl, _, _, _, _, _, mid, midT, out, outT = _sequence(pt, renderer_mod)
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl)
    r.record_moments(True)
    r.write_frame(mid)
    r.write_moments(midT)
    r.render_batch(13, _seeds(pt, 13, 2))
    assert frames_equal(r.read_frame(), out) and frames_equal(r.read_moments(), outT)
    r.close()


def test_errors_leave_frame_moments_and_the_hold_unchanged(pt, renderer_mod):
    wl = pt.scenes.m2_relit(0, W, H)
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl)
    L, rule = r._L, r.validate_rule()

    def state():
        return r.read_frame(), (r.read_moments() if moments else None)

    def refused(code, call, *a, **kw):
        before = state()
        with pytest.raises(renderer_mod.PtError) as e:
            call(*a, **kw)
        assert e.value.code == code, (code, e.value.code, call.__name__, a, kw)
        after = state()
        assert frames_equal(after[0], before[0]) and (not moments or frames_equal(after[1], before[1]))

    moments = False
    assert L.pt_history_hold(None) == -1 and L.pt_history_merge(None, C.byref(rule), None, None) == -1
    assert L.pt_history_merge(r._h, None, None, None) == -1
    r.render_batch(1, _seeds(pt, 1, 2))
    refused(-1, r.history_hold)                                     # T was never allocated
    r.record_moments(True)
    moments = True
    r.reset_frame()
    refused(-1, r.history_hold)                                     # the current image has no camera
    refused(-1, r.history_merge)                                    # no hold
    r.render_batch(1, _seeds(pt, 1, 4))
    r.history_hold()
    r.render_batch(5, _seeds(pt, 5, 2))
    nan, inf = float("nan"), float("inf")
    for kw in (dict(radius=0), dict(radius=5), dict(z_lo=-0.5), dict(z_lo=5.0), dict(z_lo=6.0), dict(z_lo=nan), dict(z_hi=nan), dict(z_hi=inf),
               dict(normal_tol=1.5), dict(normal_tol=-1.5), dict(normal_tol=nan)):
        refused(-1, r.history_merge, r.validate_rule(**kw))
    n = C.c_int64(7)
    assert L.pt_history_merge(r._h, C.byref(r.validate_rule(radius=9)), None, C.byref(n)) == -1 and n.value == 0
    r.set_buffer(14, wl.buffers[14])                                # a scene buffer uploaded since the hold
    refused(-1, r.history_merge)
    r.close()

    def held_ctx(**kw):
        q = renderer_mod.Renderer(W, H, **kw)
        q.load_workload(wl)
        q.record_moments(True)
        q.render_batch(1, _seeds(pt, 1, 4))
        return q

    for between in ("texture", "next_image", "reset_frame", "other_inputs_render", "other_inputs_write", "debug", "size"):
        r = held_ctx()
        r.history_hold()
        r.render_batch(5, _seeds(pt, 5, 2))
        code = -1
        if between == "texture":
            r.set_texture(1, wl.textures[1])
        elif between == "next_image":
            r.next_image()
        elif between == "reset_frame":
            r.reset_frame()
        elif between == "other_inputs_render":
            r.set_buffer(0, wl.buffers[0] + np.float32(0.01))
            r.render_batch(7, _seeds(pt, 7, 1))
        elif between == "other_inputs_write":
            r.set_buffer(2, np.array([3.0, 4.0, 0.0], np.float32))
            fr, T = r.read_frame(), r.read_moments()
            r.write_frame(fr)
            r.write_moments(T)
        elif between == "debug":
            r.set_buffer(4, wl.with_params(DEBUG=1.0).buffers[4])
            code = -5
        elif between == "size":
            p = wl.buffers[4].copy()
            p[2] = W / 2
            r.set_buffer(4, p)
        refused(code, r.history_merge)
        if between in ("debug", "size"):                            # the hold is still there: with the inputs back the merge goes through
            r.set_buffer(4, wl.buffers[4])
            r.history_merge()
            refused(-1, r.history_merge)                            # ... and is spent
        r.close()
    for kw in ({"shard_rank": 0, "shard_count": 2}, {"devices": [0], "first_shard": 0, "total_shards": 2}):
        r = held_ctx(**kw)
        before = r.read_frame()
        with pytest.raises(renderer_mod.PtError) as e:
            r.history_hold()
        assert e.value.code == -5 and frames_equal(r.read_frame(), before), kw
        r.close()
    # a second hold replaces the first
    r = held_ctx()
    first = state_of(r)
    r.history_hold()
    r.render_batch(5, _seeds(pt, 5, 2))
    second = state_of(r)
    r.history_hold()
    n, kappa = r.history_merge(want_kappa=True)
    assert n == 0 and (kappa == 1).all() and frames_equal(r.read_frame(), second[0]) and not frames_equal(second[0], first[0])
    r.close()


def state_of(r):
    return r.read_frame(), r.read_moments()
