"""GPU: outlier rejection (pt_despeckle, pt_despeckle_frame; include/pt_despeckle.h) against the float32 model of tests/_despeckle_model.py, bit
for bit in rgba, FRAME, T, the scale and the count: rendered images, injected images whose spikes sit on both sides of every block seam,
every special value, contexts, what the read-only call leaves alone, what follows the stored one, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import _despeckle_model as DM
from _guided_model import lum
from _reproject_model import frame_in
from conftest import frames_equal

pytestmark = pytest.mark.gpu

f32 = np.float32
INF = float("inf")
NO_MOUSE = np.array([-1.0e6, -1.0e6, 0.0], f32)
COL = np.array([1.0, 0.5, 0.25], f32)
RULE = dict(radius=1, sigmas=2.0, min_taps=4, own_z=INF, normal_tol=0.9, min_lum=0.0)


def _seeds(pt, first, n):
    return [pt.scenes.frame_seed(f) for f in range(first, first + n)]


def _fin(wl, mouse=NO_MOUSE):
    return frame_in(wl.buffers[4], wl.buffers[0], wl.buffers[1], mouse)


def _differ(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return int((a.view(np.uint32) != b.view(np.uint32)).reshape(a.shape[0], a.shape[1], -1).any(-1).sum())


def _model(F, T, feat, wl, rule, mouse=NO_MOUSE):
    return DM.despeckle(F, T, feat, _fin(wl, mouse), rule["radius"], rule["sigmas"], rule["min_taps"], rule["own_z"], rule["normal_tol"], rule["min_lum"])


def _both_calls_against_model(r, wl, moments, mouse=NO_MOUSE, tag=None, **kw):
    """pt_despeckle on the current image, held to the model and to leaving FRAME and T alone; then pt_despeckle_frame, held to the model.  Returns
    the model's results and the count"""
    rule = dict(RULE, **kw)
    crule = r.despeckle_rule(**rule)
    F, T, feat = r.read_frame(), (r.read_moments() if moments else None), r.read_features()
    wF, wT, wrgba, ws, wn = _model(F, T, feat, wl, rule, mouse)
    rgba, n, scale = r.despeckle(crule, want_scale=True)
    assert frames_equal(scale, ws), (tag, "scale", _differ(scale[..., None], ws[..., None]))
    assert frames_equal(rgba, wrgba), (tag, "rgba", _differ(rgba, wrgba))
    assert n == wn, (tag, n, wn)
    assert frames_equal(r.read_frame(), F) and (not moments or frames_equal(r.read_moments(), T)), (tag, "the read-only call wrote")
    n2, scale2 = r.despeckle_frame(crule, want_scale=True)
    F2 = r.read_frame()
    assert frames_equal(scale2, ws) and n2 == wn, (tag, "frame call", n2, wn)
    assert frames_equal(F2, wF), (tag, "FRAME", _differ(F2, wF))
    if moments:
        T2 = r.read_moments()
        assert frames_equal(T2, wT), (tag, "T", _differ(T2, wT))
    return wF, wT, ws, wn


def _context(renderer_mod, wl, moments=True, **kw):
    r = renderer_mod.Renderer(wl.W, wl.H, **kw)
    r.load_workload(wl)
    if moments:
        r.record_moments(True)
    return r


# ---------------------------------------------------------------------------------------------------------------- rendered images

@pytest.mark.parametrize("scene,w,h", [("M1", 96, 54), ("C3", 96, 54),          # two blocks across, the second partial
                                       ("M1", 130, 35), ("C3", 130, 35), ("T1", 96, 54)])      # 3 x 3 blocks, both edges partial; a textured material
def test_rendered_images_match_the_model(pt, renderer_mod, scene, w, h):
    wl = pt.scenes.m1_moving(0, w, h) if scene == "M1" else pt.scenes.build(scene, w, h)
    r = _context(renderer_mod, wl)
    r.render_batch(1, _seeds(pt, 1, 4))
    F, T = r.read_frame(), r.read_moments()
    total = 0
    for radius in (1, 2, 3):
        for own_z in (INF, 3.0):
            r.write_frame(F)
            r.write_moments(T)
            wn = _both_calls_against_model(r, wl, True, tag=(scene, w, h, radius, own_z), radius=radius, own_z=own_z)[3]
            print(f"{scene} {w}x{h} radius {radius} own_z {own_z}: {wn} of {w * h} pixels clamped")
            total += wn
    assert total > 0
    r.close()


# ---------------------------------------------------------------------------------------------------------------- injected images

def _injected(w, h, seed=3, n=4):
    """FRAME and T of n frames of a noisy surface, with one-sample spikes and converged highlights on both sides of the block seams (x = 63 | 64,
    y = 15 | 16) and in the corners, and every value the rule has a branch for"""
    rs = np.random.RandomState(seed)
    Y = (0.4 + 0.1 * rs.randn(n, h, w)).astype(f32)
    col = (Y[..., None] * COL).astype(f32)
    L = lum(col)
    fr = np.concatenate([col.sum(0, dtype=f32), np.full((h, w, 1), n, f32)], -1).astype(f32)
    T = np.stack([L.sum(0, dtype=f32), (L * L).sum(0, dtype=f32), np.full((h, w), n, f32), np.zeros((h, w), f32)], -1).astype(f32)

    def at(x, y):
        return 0 <= x < w and 0 <= y < h

    def spike(x, y, v=200.0):                                           # one more sample of v on top: a firefly
        if at(x, y):
            c = (f32(v) * COL).astype(f32)
            fr[y, x, :3] += c
            T[y, x, :2] += (lum(c), lum(c) * lum(c))

    def highlight(x, y, v=5.0):                                         # every frame said v: converged
        if at(x, y):
            c = (f32(v) * COL).astype(f32)
            fr[y, x, :3] = c * f32(n)
            T[y, x] = (lum(c) * f32(n), lum(c) * lum(c) * f32(n), n, 0.0)

    spike(0, 0); spike(w - 1, h - 1); spike(0, h - 1, 50.0); highlight(w - 1, 0)
    spike(63, 3); spike(64, 9); spike(20, 15); spike(30, 16)            # both sides of a seam: the halo is what is tested
    spike(63, 12); spike(64, 12); spike(40, 15); spike(40, 16)          # two adjacent spikes across a seam, in x and in y
    spike(63, 15); spike(64, 16, 80.0); highlight(62, 5); highlight(65, 6); highlight(10, 14); highlight(11, 17)
    for k in range(max(1, w * h // 200)):                               # and spread over the image
        (spike if k % 2 else highlight)(rs.randint(w), rs.randint(h), float(rs.choice([3.0, 20.0, 1000.0])))

    def some(k=3):
        return [(rs.randint(h), rs.randint(w)) for _ in range(k)]
    inf, nan = np.inf, np.nan
    for v in (nan, inf, -inf):                                          # in a component, as centre and as a tap of its neighbours
        for y, x in some(2):
            fr[y, x, rs.randint(3)] = v
    for y, x in some():
        fr[y, x, :3] = -fr[y, x, :3]                                    # negative components
    for y, x in some():
        fr[y, x, 1] = -3.0 * fr[y, x, 1]
    for a in (0.0, 0.5, inf, -1.0, nan):                                # A
        for y, x in some(2):
            fr[y, x, 3] = a
    for y, x in some(2):
        fr[y, x, :3] = (f32(1.0e20) * COL) * fr[y, x, 3]                # l*l overflows in Q
        spike(x + 1, y)
    if w >= 30 and h >= 7:
        fr[2:6, 20:26, :3] = (f32(1.0e20) * COL) * f32(n)
        fr[2:6, 20:26, 3] = n
    for cnt in (0.0, 1.0, 2.0, 7.0, inf, nan):                          # T.n: 0, 1, 2 and n != A, beside a spike so that step 5 is reached
        for y, x in some(2):
            spike(x, y, 100.0)
            T[y, x, 2] = cnt
    for y, x in some(2):
        spike(x, y, 100.0)
        T[y, x, rs.randint(2)] = rs.choice([nan, inf])
    return fr, T


@pytest.mark.parametrize("w,h", [(64, 16), (65, 17), (100, 7), (5, 3), (1, 1)])      # one exact block; one pixel into the next in both directions; ...
@pytest.mark.parametrize("own_z", [INF, 3.0])
def test_injected_images_match_the_model(pt, renderer_mod, w, h, own_z):
    wl = pt.scenes.build("C3", w, h)
    r = _context(renderer_mod, wl)
    F, T = _injected(w, h)
    clamped = []
    for radius, sigmas, min_taps, min_lum in ((1, 2.0, 4, 0.0), (2, 3.0, 2, 0.0), (3, 0.0, 48, 0.0), (3, 2.0, 4, 0.5), (2, 2.0, 24, 0.0)):
        r.write_frame(F)
        r.write_moments(T)
        got = _both_calls_against_model(r, wl, True, tag=(w, h, radius, sigmas, own_z), radius=radius, sigmas=sigmas, min_taps=min_taps, own_z=own_z, min_lum=min_lum)
        clamped.append(got[3])
    print(f"injected {w}x{h} own_z {own_z}: clamped {clamped}")
    if w * h >= 64 * 16:
        assert clamped[0] > 0 and clamped[1] > 0
    r.close()


def test_own_z_decides_between_a_spike_and_a_highlight_on_the_device(pt, renderer_mod):
    """what step 5 is for, on the device: with own_z = 3 the converged highlights of the injected image stay and its one-sample spikes go"""
    w, h = 65, 17
    wl = pt.scenes.build("C3", w, h)
    r = _context(renderer_mod, wl)
    F, T = _injected(w, h)
    r.write_frame(F)
    r.write_moments(T)
    _, n_inf, s_inf = r.despeckle(r.despeckle_rule(**RULE), want_scale=True)
    _, n_3, s_3 = r.despeckle(r.despeckle_rule(**dict(RULE, own_z=3.0)), want_scale=True)
    assert 0 < n_3 < n_inf and ((s_3 == 1) | (s_3 == s_inf)).all()
    r.close()


def test_the_overlay_and_a_sky_region(pt, renderer_mod):
    w, h = 96, 54
    wl = pt.scenes.build("C1", w, h)                                    # spheres under an open sky
    r = _context(renderer_mod, wl)
    r.render_batch(1, _seeds(pt, 1, 4))
    feat = r.read_features()
    sky = feat[..., 7].copy().view(np.int32) == -1
    F, T = r.read_frame(), r.read_moments()
    ys, xs = np.nonzero(sky[1:-1, 1:-1] & sky[:-2, 1:-1] & sky[2:, 1:-1] & sky[1:-1, :-2] & sky[1:-1, 2:])
    assert len(ys), "C1 has no sky region at this size"
    sy, sx = int(ys[0]) + 1, int(xs[0]) + 1
    F[sy, sx, :3] *= f32(40.0)                                          # a spike in the sky, and one on a surface under the mouse
    K = DM.despeckle(F, T, feat, _fin(wl), 1, 2.0, 4, INF, 0.9, 0.0, detail=True)[5]["K"]
    hy, hx = [int(v[0]) for v in np.nonzero(~sky & (K == 8))]         # a surface pixel whose eight neighbours all count
    F[hy, hx, :3] = f32(500.0) * F[hy, hx, 3]
    for mouse in (NO_MOUSE, np.array([hx, hy, 0.0], f32)):
        r.set_buffer(2, mouse)
        r.write_frame(F)
        r.write_moments(T)
        wF, wT, ws, wn = _both_calls_against_model(r, wl, True, mouse, tag=("overlay", tuple(mouse)))
        assert ws[sy, sx] < 1
        assert (ws[hy, hx] == 1) == (mouse is not NO_MOUSE)
    r.close()


def test_without_moments_the_test_of_own_z_is_off_and_t_stays_unallocated(pt, renderer_mod):
    w, h = 65, 17
    wl = pt.scenes.build("C3", w, h)
    r = _context(renderer_mod, wl, moments=False)
    F, _ = _injected(w, h)
    r.write_frame(F)
    wF, wT, ws, wn = _both_calls_against_model(r, wl, False, tag="no T")
    assert wn > 0 and wT is None
    with pytest.raises(renderer_mod.PtError) as e:                      # T was never allocated, and still is not
        r.history_hold()
    assert e.value.code == -1 and "never allocated" in str(e.value)
    r.close()


# ---------------------------------------------------------------------------------------------------------------- what the calls leave and what follows

W, H = 96, 54


def _rendered(pt, renderer_mod, **kw):
    wl = pt.scenes.build("C3", W, H)
    r = _context(renderer_mod, wl, **kw)
    r.render_batch(1, _seeds(pt, 1, 4))
    return r, wl


def test_the_read_only_call_leaves_the_image_its_camera_and_the_caches(pt, renderer_mod):
    r, wl = _rendered(pt, renderer_mod)
    twin, _ = _rendered(pt, renderer_mod)
    before = r.read_frame(), r.read_moments(), r.read_features()
    rgba, n = r.despeckle()
    assert n > 0
    assert frames_equal(r.read_frame(), before[0]) and frames_equal(r.read_moments(), before[1]) and frames_equal(r.read_features(), before[2])
    moved = wl.buffers[0] + np.array([0.02, 0.0, 0.01], f32)           # the image still has the camera it was rendered from
    kept = []
    for q in (r, twin):
        q.set_buffer(0, moved)
        kept.append(q.reproject_frame())
    assert kept[0] == kept[1] and kept[0] > 0
    assert frames_equal(r.read_frame(), twin.read_frame()) and frames_equal(r.read_moments(), twin.read_moments())
    r.close()
    twin.close()


def test_consumers_and_later_frames_see_the_stored_image(pt, renderer_mod):
    r, wl = _rendered(pt, renderer_mod)
    F, T, feat = r.read_frame(), r.read_moments(), r.read_features()
    wF, wT, _, _, wn = _model(F, T, feat, wl, RULE)
    assert r.despeckle_frame() == wn and wn > 0
    twin = _context(renderer_mod, wl)
    twin.write_frame(wF)
    twin.write_moments(wT)
    assert frames_equal(r.denoise_guided(), twin.denoise_guided())
    for q in (r, twin):
        q.render_batch(5, _seeds(pt, 5, 2))
    assert frames_equal(r.read_frame(), twin.read_frame()) and frames_equal(r.read_moments(), twin.read_moments())
    r.close()
    twin.close()


def test_a_call_under_a_running_frame_stream_equals_one_after_synchronize(pt, renderer_mod):
    got = []
    for sync in (False, True):
        wl = pt.scenes.build("C3", W, H)
        r = _context(renderer_mod, wl)
        r.render_batch_async(1, _seeds(pt, 1, 4))
        if sync:
            r.synchronize()
        rgba, n, scale = r.despeckle(want_scale=True)
        n2 = r.despeckle_frame()
        got.append((rgba, scale, r.read_frame(), r.read_moments(), n, n2))
        r.close()
    assert got[0][4] == got[1][4] == got[0][5] == got[1][5] and got[0][4] > 0
    for a, b in zip(got[0][:4], got[1][:4]):
        assert frames_equal(a, b)


def test_multi_stream_context_equals_one_stream(pt, renderer_mod):
    def sequence(**kw):
        r, wl = _rendered(pt, renderer_mod, **kw)
        rgba, n, scale = r.despeckle(r.despeckle_rule(own_z=3.0), want_scale=True)
        same = r.read_frame()
        n2, scale2 = r.despeckle_frame(r.despeckle_rule(radius=2), want_scale=True)
        out = rgba, scale, same, scale2, r.read_frame(), r.read_moments(), n, n2
        r.close()
        return out
    one = sequence()
    assert one[6] > 0 and one[7] > 0
    for kw in ({"devices": [0, 0]}, {"devices": [0]}):
        got = sequence(**kw)
        assert got[6:] == one[6:], kw
        for a, b in zip(got[:6], one[:6]):
            assert frames_equal(a, b), kw


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_every_refusal_leaves_frame_and_moments_unchanged(pt, renderer_mod):
    wl = pt.scenes.build("C3", W, H)
    r = _context(renderer_mod, wl, moments=False)
    L, rule = r._L, r.despeckle_rule()
    moments = False

    def refused(code, call, *a, **kw):
        before = r.read_frame(), (r.read_moments() if moments else None)
        with pytest.raises(renderer_mod.PtError) as e:
            call(*a, **kw)
        assert e.value.code == code, (code, e.value.code, str(e.value), call.__name__, a, kw)
        assert frames_equal(r.read_frame(), before[0]) and (not moments or frames_equal(r.read_moments(), before[1]))
        return str(e.value)

    n = C.c_int64(7)
    assert L.pt_despeckle(None, C.byref(rule), None, None, C.byref(n)) == -1 and n.value == 0
    assert L.pt_despeckle_frame(None, C.byref(rule), None, None) == -1
    assert L.pt_despeckle(r._h, None, None, None, None) == -1 and L.pt_despeckle_frame(r._h, None, None, None) == -1
    r.render_batch(1, _seeds(pt, 1, 2))
    nan, inf = float("nan"), INF
    for call in (r.despeckle, r.despeckle_frame):
        for kw in (dict(radius=0), dict(radius=4), dict(sigmas=-0.5), dict(sigmas=inf), dict(sigmas=nan), dict(min_taps=1), dict(min_taps=9), dict(radius=3, min_taps=49),
                   dict(own_z=0.0), dict(own_z=-1.0), dict(own_z=nan), dict(normal_tol=1.5), dict(normal_tol=-1.5), dict(normal_tol=nan), dict(min_lum=-0.5),
                   dict(min_lum=inf), dict(min_lum=nan)):
            assert call.__name__ in refused(-1, call, r.despeckle_rule(**kw)), kw
        assert "never allocated" in refused(-1, call, r.despeckle_rule(own_z=3.0))      # a finite own_z needs T
    n.value = 7
    assert L.pt_despeckle_frame(r._h, C.byref(r.despeckle_rule(radius=9)), None, C.byref(n)) == -1 and n.value == 0
    r.record_moments(True)
    moments = True
    r.render_batch(3, _seeds(pt, 3, 2))
    for call in (r.despeckle, r.despeckle_frame):
        p = wl.buffers[4].copy()
        p[2] = W / 2
        r.set_buffer(4, p)                                              # Parameters that do not match the image size
        refused(-1, call, r.despeckle_rule(own_z=3.0))
        r.set_buffer(4, wl.with_params(DEBUG=1.0).buffers[4])
        assert call.__name__ in refused(-5, call)
        r.set_buffer(4, wl.buffers[4])
    assert r.despeckle_frame(r.despeckle_rule(own_z=3.0)) >= 0          # with the inputs back both go through
    r.close()
    bare = renderer_mod.Renderer(W, H)                                  # Parameters / ORIGIN / ROTATION not set
    for call in (bare.despeckle, bare.despeckle_frame):
        with pytest.raises(renderer_mod.PtError) as e:
            call()
        assert e.value.code == -1
    bare.close()
    for kw in ({"shard_rank": 0, "shard_count": 2}, {"devices": [0], "first_shard": 0, "total_shards": 2}):
        q = _context(renderer_mod, wl, **kw)
        q.render_batch(1, _seeds(pt, 1, 2))
        before = q.read_frame()
        for call in (q.despeckle, q.despeckle_frame):
            with pytest.raises(renderer_mod.PtError) as e:
                call()
            assert e.value.code == -5, (kw, str(e.value))
        assert frames_equal(q.read_frame(), before), kw
        q.close()
