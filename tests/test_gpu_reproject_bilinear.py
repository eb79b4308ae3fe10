"""GPU: reprojection with bilinear taps (pt_reproject_frame_bilinear; include/pt_reproject_bilinear.h) held to the float32 model of
tests/_reproject_bilinear_model.py bit for bit in FRAME, T and both counts, on the feature records read from the device and images injected through
pt_write_frame / pt_write_moments; then what needs no model: the identity against pt_reproject_frame on a twin context, the kept set, contexts,
later renders, errors, the no-op."""
import ctypes as C

import numpy as np
import pytest

from _reproject_bilinear_model import reproject_bilinear as model
from _reproject_model import cam_rot, frame_in, material_flags
from conftest import frames_equal
from test_gpu_reproject import move

pytestmark = pytest.mark.gpu

W, H = 96, 54
OFF = np.array([-1.0e6, -1.0e6, 0.0], np.float32)
SCENES = {"M1-plain": ("M1", dict(textured=False), 0.0), "M1-textured": ("M1", dict(textured=True), 0.05), "C3": ("C3", dict(subdiv=2), 0.0)}


def _turn(origin, rotation, dx=0.0, dy=0.0, dz=0.0):
    return np.asarray(origin, np.float32)[:3].copy(), (np.asarray(rotation, np.float32)[:3] + np.array([dx, dy, dz], np.float32)).astype(np.float32)


# a sub-pixel translation; rotations (pitch, yaw and roll, both ways) that bring taps off every image border; a dolly forward
MOVES = {"sub-pixel": lambda A: move(*A, forward=0.004, strafe=0.02), "turn": lambda A: _turn(*A, 0.02, 0.03, 0.06),
         "turn-back": lambda A: _turn(*A, -0.02, -0.03, -0.06), "dolly": lambda A: move(*A, forward=0.15)}


def _open(pt, renderer_mod, scene, w=W, h=H, wl=None, **kw):
    name, skw, floor = SCENES[scene]
    wl = pt.scenes.build(name, w, h, **skw) if wl is None else wl
    r = renderer_mod.Renderer(w, h, **kw)
    r.load_workload(wl)
    return r, wl, floor


def _setcam(r, cam, mouse=OFF):
    r.set_buffer(0, np.asarray(cam[0], np.float32))
    r.set_buffer(1, np.asarray(cam[1], np.float32))
    r.set_buffer(2, np.asarray(mouse, np.float32))


def _image(w, h, seed=3, bad=True):
    """a FRAME of random means and counts 1 .. 99 and a T beside it; bad: NaN, inf and zero-count pixels in both"""
    rs = np.random.RandomState(seed)
    cnt = rs.randint(1, 100, size=(h, w, 1)).astype(np.float32)
    fr = np.concatenate([rs.rand(h, w, 3).astype(np.float32) * cnt, cnt], -1)
    n = rs.randint(1, 100, size=(h, w)).astype(np.float32)
    Y = rs.rand(h, w).astype(np.float32)
    T = np.stack([n * Y, n * Y * Y * (1.0 + rs.rand(h, w) * 0.5), n, np.zeros_like(n)], -1).astype(np.float32)
    if bad:
        fr[1, 7, 0] = np.nan
        fr[2, 30, 1:3] = np.inf
        fr[3:5, 40:44] = (1.0, 2.0, 3.0, 0.0)
        fr[5, 50, 3] = -3.0
        T[1, 12, 0] = np.nan
        T[2, 20, 1] = np.inf
        T[3:6, 60:63, 2] = 0.0
        T[4, 70, 2] = -1.0
        T[5, 80, 2] = np.nan
    return fr, T


def _want(r, wl, rn, rh, fr, T, A, B, mouse_b, mh, dt, nt, snap, allm, floor):
    cos = lambda x: r.debug_math("cos", x)      # noqa: E731  (the shader's own functions, as k_frame_setup calls them)
    sin = lambda x: r.debug_math("sin", x)      # noqa: E731
    fin_a = frame_in(wl.buffers[4], A[0], A[1], OFF)
    fin_b = frame_in(wl.buffers[4], B[0], B[1], mouse_b)
    return model(rn, rh, fr, T, fin_a, fin_b, material_flags(wl.buffers[14]), cam_rot(A[1], cos, sin), mh, dt, nt, snap, allm, floor, detail=True)


def _bits(a, b):
    return int((np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)).any(-1).sum())


@pytest.mark.parametrize("w,h", [(100, 7), (130, 33)])      # 100 x 7: a partial block of columns, below a block's 16 rows; 130 x 33: three by three blocks, partial both ways
@pytest.mark.parametrize("scene", list(SCENES))
def test_gpu_matches_the_model(pt, renderer_mod, scene, w, h):
    r, wl, floor = _open(pt, renderer_mod, scene, w, h)
    A = (wl.buffers[0], wl.buffers[1])
    _setcam(r, A)
    rh = r.read_features()
    vd = material_flags(wl.buffers[14])
    assert vd.any() == (scene == "C3")
    mouse = np.array([w * 0.3, h * 0.6, 0.0], np.float32)
    # (T allocated, overlay, injected bad pixels, rule): T is allocated by the first pt_write_moments, so the runs without it come first
    variants = [(False, OFF, True, dict(mh=64.0, dt=0.02, nt=0.9, snap=1.0 / 64, allm=False)),
                (True, mouse, True, dict(mh=64.0, dt=0.02, nt=0.9, snap=1.0 / 64, allm=False)),
                (True, OFF, False, dict(mh=10.0, dt=0.05, nt=0.5, snap=0.0, allm=True))]
    borders = np.zeros(4, np.int64)
    for with_t, mouse_b, bad, rule in variants:
        fr, T = _image(w, h, bad=bad)
        for name, mv in MOVES.items():
            B = mv(A)
            _setcam(r, A)
            r.write_frame(fr)                                   # the image's camera: A
            if with_t:
                r.write_moments(T)
            _setcam(r, B, mouse_b)
            rn = r.read_features()
            kept, blended = r.reproject_frame_bilinear(rule["mh"], rule["dt"], rule["nt"], rule["snap"], rule["allm"], floor)
            got, gotT = r.read_frame(), r.read_moments()
            want, wantT, wkept, wblended, d = _want(r, wl, rn, rh, fr, T if with_t else None, A, B, mouse_b, floor=floor, **rule)
            tag = (scene, w, h, name, with_t, rule)
            print(f"{scene} {w}x{h} {name} T={with_t}: kept {kept} / {wkept}, blended {blended} / {wblended} of {w * h}")
            assert frames_equal(got, want), (tag, _bits(got, want))
            if with_t:
                assert frames_equal(gotT, wantT), (tag, _bits(gotT, wantT))
            else:
                assert not gotT.any(), tag
            assert (kept, blended) == (wkept, wblended) and 0 < blended <= kept <= w * h, (tag, kept, wkept, blended, wblended)
            if scene == "C3" and not rule["allm"]:
                assert kept < w * h, tag                        # the glass and the metal restart
            if name.startswith("turn"):                         # pixels whose taps reach past the left, right, top and bottom border
                ok = d["taps"] > 0
                borders += [int((ok & (d["sx"] < 0.5)).sum()), int((ok & (d["sx"] > w - 0.5)).sum()), int((ok & (d["sy"] < 0.5)).sum()),
                            int((ok & (d["sy"] > h - 0.5)).sum())]
            if floor > 0 and name == "dolly" and not bad:       # the demodulated carry is another result than the plain one where the texel changed
                plain = _want(r, wl, rn, rh, fr, T, A, B, mouse_b, floor=0.0, **rule)
                assert plain[2] == wkept and not frames_equal(plain[0], want), tag
    assert (borders > 0).all(), (scene, w, h, borders)
    r.close()


def _twins(pt, renderer_mod, scene, w=W, h=H):
    r, wl, floor = _open(pt, renderer_mod, scene, w, h)
    twin, _, _ = _open(pt, renderer_mod, scene, w, h, wl=wl)
    return r, twin, wl, floor


def _identity(r, twin, wl, w, h, floor):
    """the camera unchanged: pt_reproject_frame_bilinear on r against pt_reproject_frame / pt_reproject_frame_demod on its twin"""
    fr, T = _image(w, h)
    for x in (r, twin):
        x.write_frame(fr)
        x.write_moments(T)
    kept, blended = r.reproject_frame_bilinear(albedo_floor=floor)
    wkept = twin.reproject_frame(albedo_floor=floor if floor > 0 else None)
    got, want = r.read_frame(), twin.read_frame()
    assert frames_equal(got, want), (w, h, floor, _bits(got, want))
    assert frames_equal(r.read_moments(), twin.read_moments()), (w, h, floor)
    assert kept == wkept and blended == 0 and 0 < kept < w * h, (kept, wkept, blended)


@pytest.mark.parametrize("w,h", [(100, 7), (130, 33)])
def test_unchanged_camera_equals_the_nearest_calls_on_a_twin(pt, renderer_mod, w, h):
    for scene in ("M1-textured", "C3"):
        r, twin, wl, _ = _twins(pt, renderer_mod, scene, w, h)
        for floor in (0.0, 0.05):
            _identity(r, twin, wl, w, h, floor)
        r.close()
        twin.close()


def test_unchanged_camera_at_full_size(pt, renderer_mod):
    """C3 at 1920 x 1080: the identity on every pixel also shows that the default snap clears the rounding of sx and sy"""
    w, h = 1920, 1080
    wl = pt.scenes.build("C3", w, h)
    r, _, _ = _open(pt, renderer_mod, "C3", w, h, wl=wl)
    twin, _, _ = _open(pt, renderer_mod, "C3", w, h, wl=wl)
    _identity(r, twin, wl, w, h, 0.0)
    r.close()
    twin.close()


@pytest.mark.parametrize("scene", ["M1-textured", "C3"])
def test_keeps_every_pixel_the_nearest_call_keeps(pt, renderer_mod, scene):
    r, twin, wl, floor = _twins(pt, renderer_mod, scene)
    A = (wl.buffers[0], wl.buffers[1])
    fr, T = _image(W, H)
    for name, mv in MOVES.items():
        for x in (r, twin):
            _setcam(x, A)
            x.write_frame(fr)
            x.write_moments(T)
            _setcam(x, mv(A))
        kept, blended = r.reproject_frame_bilinear(albedo_floor=floor)
        near = twin.reproject_frame(albedo_floor=floor if floor > 0 else None)
        got, want = r.read_frame(), twin.read_frame()
        print(f"{scene} {name}: nearest keeps {near}, bilinear {kept} (blended {blended}) of {W * H}")
        assert kept >= near > 0 and 0 < blended <= kept, (scene, name, kept, near, blended)
        assert (got[..., 3] > 0)[want[..., 3] > 0].all(), (scene, name)
        assert kept == int((got[..., 3] > 0).sum())
    r.close()
    twin.close()


def _sequence(pt, r, wl, floor):
    A = (wl.buffers[0], wl.buffers[1])
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 7)]
    r.render_adaptive(1, seeds[:4], 0.0, 0.0, min_frames=100)
    _setcam(r, move(*A, forward=0.04, strafe=0.03, yaw=0.03))
    kept, blended = r.reproject_frame_bilinear(max_history=3.0, albedo_floor=floor)
    mid, midT = r.read_frame(), r.read_moments()
    n = r.render_adaptive(5, seeds[4:6], 0.0, 1e30, min_frames=3)
    return kept, blended, mid, midT, n, r.read_frame()


def test_multi_stream_context_equals_one_stream(pt, renderer_mod):
    out = []
    for kw in ({}, {"devices": [0, 0]}, {"devices": [0]}):
        r, wl, floor = _open(pt, renderer_mod, "M1-textured", **kw)
        out.append(_sequence(pt, r, wl, floor))
        r.close()
    k0, b0, m0, t0, n0, f0 = out[0]
    assert 0 < b0 <= k0 < W * H and 0 < n0 < W * H
    for k1, b1, m1, t1, n1, f1 in out[1:]:
        assert (k0, b0, n0) == (k1, b1, n1)
        assert frames_equal(m0, m1) and frames_equal(t0, t1) and frames_equal(f0, f1)


def test_renders_after_the_call_equal_renders_on_its_written_image(pt, renderer_mod):
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 10)]
    r, wl, _ = _open(pt, renderer_mod, "C3")
    A = (wl.buffers[0], wl.buffers[1])
    B = move(*A, forward=0.02, strafe=-0.02, yaw=-0.02)
    r.render_adaptive(1, seeds[:4], 0.0, 0.0, min_frames=100)
    _setcam(r, B)
    kept, blended = r.reproject_frame_bilinear()
    assert 0 < blended <= kept < W * H
    mid, midT = r.read_frame(), r.read_moments()
    n = r.render_adaptive(5, seeds[4:9], 0.5, 0.0, min_frames=3)
    got, gotT = r.read_frame(), r.read_moments()
    r.close()
    r2, _, _ = _open(pt, renderer_mod, "C3", wl=wl)
    _setcam(r2, B)
    r2.write_frame(mid)
    r2.write_moments(midT)
    assert r2.render_adaptive(5, seeds[4:9], 0.5, 0.0, min_frames=3) == n
    want, wantT = r2.read_frame(), r2.read_moments()
    r2.close()
    assert frames_equal(got, want) and frames_equal(gotT, wantT)


def test_errors_leave_frame_and_t_unchanged(pt, renderer_mod):
    PtError, Rule = renderer_mod.PtError, renderer_mod.ReprojectBilinearRule
    r, wl, _ = _open(pt, renderer_mod, "M1-textured")
    A = (wl.buffers[0], wl.buffers[1])
    fr, T = _image(W, H)
    r.write_frame(fr)
    r.write_moments(T)
    _setcam(r, move(*A, forward=0.03))
    nan, inf = float("nan"), float("inf")

    def same():
        return frames_equal(r.read_frame(), fr) and frames_equal(r.read_moments(), T)

    def raw(rule, ctx=True):
        n, nb = C.c_int64(7), C.c_int64(7)
        rc = r._L.pt_reproject_frame_bilinear(r._h if ctx else None, C.byref(rule) if rule is not None else None, C.byref(n), C.byref(nb))
        return rc, n.value, nb.value
    good = dict(max_history=64.0, depth_tol=0.02, normal_tol=0.9, snap=1.0 / 64, albedo_floor=0.0, flags=0)
    bad = [dict(max_history=0.5), dict(max_history=nan), dict(depth_tol=0.0), dict(depth_tol=-1.0), dict(depth_tol=nan), dict(normal_tol=1.5),
           dict(normal_tol=-1.5), dict(normal_tol=nan), dict(flags=2), dict(snap=-0.01), dict(snap=0.5), dict(snap=nan), dict(snap=inf),
           dict(albedo_floor=-0.1), dict(albedo_floor=nan), dict(albedo_floor=inf)]
    for kw in bad:
        assert raw(Rule(**{**good, **kw})) == (-1, 0, 0), kw
        assert same(), kw
    assert raw(None) == (-1, 0, 0) and raw(Rule(**good), ctx=False) == (-1, 0, 0) and same()
    assert r._L.pt_reproject_frame_bilinear(r._h, None, None, None) == -1
    with pytest.raises(PtError) as e:
        r.reproject_frame_bilinear(snap=0.75)
    assert e.value.code == -1
    p = wl.buffers[4].copy()
    p[10] = 1.0                                                 # DEBUG
    r.set_buffer(4, p)
    assert raw(Rule(**good)) == (-5, 0, 0) and same()
    p = wl.buffers[4].copy()
    p[2] = W / 2                                                # resolution no longer the image's
    r.set_buffer(4, p)
    assert raw(Rule(**good)) == (-1, 0, 0) and same()
    r.set_buffer(4, wl.buffers[4])
    r.set_buffer(14, wl.buffers[14])                            # a scene upload since the camera was recorded (even the same contents)
    assert raw(Rule(**good)) == (-1, 0, 0) and same()
    r.write_frame(fr)                                           # (a written image has no moments: T again)
    r.write_moments(T)
    r.set_texture(0, wl.sky)
    assert raw(Rule(**good)) == (-1, 0, 0) and same()
    r.write_frame(fr)                                           # the camera again: the call goes through, with null count pointers too
    assert r._L.pt_reproject_frame_bilinear(r._h, C.byref(Rule(**good)), None, None) == 0 and not same()
    r.close()
    for kw in ({"shard_rank": 0, "shard_count": 2}, {"devices": [0], "first_shard": 0, "total_shards": 2}):
        r, wl, _ = _open(pt, renderer_mod, "M1-textured", **kw)
        r.render_batch(1, [pt.scenes.frame_seed(1)])
        before = r.read_frame()
        with pytest.raises(PtError) as e:
            r.reproject_frame_bilinear()
        assert e.value.code == -5, kw
        assert frames_equal(r.read_frame(), before)
        r.close()


def test_an_image_without_a_camera_is_left_alone(pt, renderer_mod):
    wl = pt.scenes.build("C2", W, H)
    r = renderer_mod.Renderer(W, H)
    fr, _ = _image(W, H)
    r.write_frame(fr)                                           # no Parameters yet: no camera
    r.load_workload(wl)
    assert r.reproject_frame_bilinear() == (0, 0) and frames_equal(r.read_frame(), fr)
    r.render_batch(1, [pt.scenes.frame_seed(1)])
    r.reset_frame()
    _setcam(r, move(wl.buffers[0], wl.buffers[1], forward=0.03))
    assert r.reproject_frame_bilinear() == (0, 0) and not r.read_frame().any()
    r.render_batch(1, [pt.scenes.frame_seed(1)])
    r.next_image()
    assert r.reproject_frame_bilinear() == (0, 0) and not r.read_frame().any()
    r.close()
