"""GPU: reprojection across a camera move (pt_reproject_frame; include/pt_reproject.h) against the float32 model of tests/_reproject_model.py, on
the feature records of real scenes and FRAMEs injected through pt_write_frame; T, later renders, contexts, errors, the no-op, and its effect on noise."""
import ctypes as C
import math

import numpy as np
import pytest

from _adaptive_model import Model, select
from _reproject_model import cam_rot, frame_in, material_flags, reproject as model
from conftest import frames_equal, rmse

pytestmark = pytest.mark.gpu

W, H = 96, 54


def move(origin, rotation, forward=0.0, strafe=0.0, yaw=0.0):
    """one step of the reference's functions.move (dispatch.java:738-777): W / A keys scaled to `forward` / `strafe`, LEFT to `yaw`"""
    cam = [float(v) for v in origin[:3]]
    rot = [float(v) for v in rotation[:3]]
    cam[0] -= forward * math.cos(rot[1] + math.pi / 2); cam[2] += forward * math.sin(rot[1] + math.pi / 2)
    cam[0] += strafe * math.cos(rot[1]); cam[2] -= strafe * math.sin(rot[1])
    rot[1] += yaw
    return np.array(cam, np.float32), np.array(rot, np.float32)


def _ctx(pt, renderer_mod, name="C2", **kw):
    wl = pt.scenes.build(name, W, H)
    r = renderer_mod.Renderer(W, H, **kw)
    r.load_workload(wl)
    return r, wl


def _inject(seed=3):
    rs = np.random.RandomState(seed)
    cnt = rs.randint(1, 100, size=(H, W, 1)).astype(np.float32)
    fr = np.concatenate([rs.rand(H, W, 3).astype(np.float32) * cnt, cnt], -1)
    fr[5, 7, 0] = np.nan
    fr[9, 30, 1:3] = np.inf
    fr[20:23, 40:44] = (1.0, 2.0, 3.0, 0.0)
    return fr


def _setcam(r, origin, rotation):
    r.set_buffer(0, np.asarray(origin, np.float32))
    r.set_buffer(1, np.asarray(rotation, np.float32))


def _want(r, wl, rn, rh, fr, A, B, mouse_b, T=None, mh=64.0, dt=0.02, nt=0.9, allm=False):
    cos = lambda x: r.debug_math("cos", x)      # noqa: E731  (the shader's own functions, as k_frame_setup calls them)
    sin = lambda x: r.debug_math("sin", x)      # noqa: E731
    fin_a = frame_in(wl.buffers[4], A[0], A[1], wl.buffers[2])
    fin_b = frame_in(wl.buffers[4], B[0], B[1], mouse_b)
    return model(rn, rh, fr, T, fin_a, fin_b, material_flags(wl.buffers[14]), cam_rot(A[1], cos, sin), mh, dt, nt, allm)


CASES = [dict(mh=64.0, dt=0.02, nt=0.9, allm=False), dict(mh=10.0, dt=0.05, nt=0.5, allm=True)]


@pytest.mark.parametrize("scene", ["C1", "C2", "C3", "T1", "C6"])
def test_gpu_matches_the_model(pt, renderer_mod, scene):
    r, wl = _ctx(pt, renderer_mod, scene)
    A = (wl.buffers[0], wl.buffers[1])
    rh = r.read_features()
    fr = _inject()
    for step, (fwd, strafe, yaw) in enumerate([(0.03, 0.02, 0.02), (-0.05, 0.0, -0.03)]):
        B = move(*A, forward=fwd, strafe=strafe, yaw=yaw)
        mouse_b = np.array([30.0, 17.0, 0.0] if step else [-1.0e6, -1.0e6, 0.0], np.float32)
        for case in CASES:
            _setcam(r, *A)
            r.set_buffer(2, wl.buffers[2])
            r.write_frame(fr)                                   # the image's camera: A
            _setcam(r, *B)
            r.set_buffer(2, mouse_b)
            rn = r.read_features()
            kept = r.reproject_frame(case["mh"], case["dt"], case["nt"], case["allm"])
            got = r.read_frame()
            want, _, wkept = _want(r, wl, rn, rh, fr, A, B, mouse_b, **case)
            assert frames_equal(got, want), (scene, step, case, int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum()))
            assert kept == wkept and 0 < kept < W * H, (scene, step, case, kept, wkept)
    r.close()


def test_unchanged_camera_is_the_identity(pt, renderer_mod):
    for scene in ("C2", "C3"):
        r, wl = _ctx(pt, renderer_mod, scene)
        A = (wl.buffers[0], wl.buffers[1])
        fr = _inject()
        fr[..., :3] *= np.float32(0.5)
        fr[..., 3] = np.minimum(fr[..., 3], 50.0)              # below the cap
        r.write_frame(fr)
        kept = r.reproject_frame()
        got = r.read_frame()
        f = r.read_features()
        want, _, wkept = _want(r, wl, f, f, fr, A, A, wl.buffers[2])
        assert frames_equal(got, want) and kept == wkept
        keep = got[..., 3] > 0
        assert np.array_equal(got[keep].view(np.uint32), fr[keep].view(np.uint32))       # every pixel that is kept is unchanged
        if scene == "C2":
            assert kept > 0.95 * (W * H - 12 - 4)               # everything but the injected bad pixels (C2 is all diffuse)
        r.close()


def test_statistics_are_carried(pt, renderer_mod):
    """T is reprojected with FRAME: after 4 adaptive frames on every pixel (n = 4), the pixels that kept their history are not below min_frames 4,
    the others (n = 0) are; with an absolute error of 1e30 nothing else is selected"""
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 9)]
    r, wl = _ctx(pt, renderer_mod, "C2")
    A = (wl.buffers[0], wl.buffers[1])
    assert r.render_adaptive(1, seeds[:4], 0.0, 0.0, min_frames=100) == W * H
    rh = r.read_features()
    fr = r.read_frame()
    B = move(*A, forward=0.04, strafe=0.03, yaw=0.03)
    _setcam(r, *B)
    rn = r.read_features()
    kept = r.reproject_frame()
    want, _, wkept = _want(r, wl, rn, rh, fr, A, B, wl.buffers[2])
    assert kept == wkept and frames_equal(r.read_frame(), want)
    n = r.render_adaptive(5, seeds[4:6], 0.0, 1e30, min_frames=4)
    assert n == W * H - kept and 0 < n < W * H // 2
    # without the reprojection of T every pixel would still have n = 4 (nothing selected) or, zeroed, every pixel
    r.close()


def _sequence(r, wl, seeds):
    A = (wl.buffers[0], wl.buffers[1])
    r.render_adaptive(1, seeds[:4], 0.0, 0.0, min_frames=100)
    _setcam(r, *move(*A, forward=0.04, strafe=0.03, yaw=0.03))
    kept = r.reproject_frame(max_history=3.0)                 # n = 4 capped to 3: the kept pixels are not below min_frames 3
    mid = r.read_frame()
    n = r.render_adaptive(5, seeds[4:6], 0.0, 1e30, min_frames=3)
    return kept, mid, n, r.read_frame()


def test_multi_stream_context_equals_one_stream(pt, renderer_mod):
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 9)]
    out = []
    for kw in ({}, {"devices": [0, 0]}, {"devices": [0]}):      # [0]: a group of one stream, whose context holds the whole image
        r, wl = _ctx(pt, renderer_mod, "C3", **kw)
        out.append(_sequence(r, wl, seeds))
        r.close()
    k0, m0, n0, f0 = out[0]
    assert 0 < k0 < W * H and n0 == W * H - k0
    for kw, (k1, m1, n1, f1) in zip(({"devices": [0, 0]}, {"devices": [0]}), out[1:]):
        assert k0 == k1 and n0 == n1, kw
        assert frames_equal(m0, m1) and frames_equal(f0, f1), kw


def test_renders_after_a_reprojection_equal_renders_on_its_written_image(pt, renderer_mod):
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 10)]
    r, wl = _ctx(pt, renderer_mod, "C3")
    A = (wl.buffers[0], wl.buffers[1])
    B = move(*A, forward=0.02, strafe=-0.02, yaw=-0.02)
    r.render_batch(1, seeds[:4])
    _setcam(r, *B)
    r.reproject_frame()
    mid = r.read_frame()
    r.render_batch(5, seeds[4:9])
    got = r.read_frame()
    r.close()
    r2, _ = _ctx(pt, renderer_mod, "C3")
    _setcam(r2, *B)
    r2.write_frame(mid)
    r2.render_batch(5, seeds[4:9])
    want = r2.read_frame()
    r2.close()
    assert frames_equal(got, want)


def test_errors_leave_frame_unchanged(pt, renderer_mod):
    r, wl = _ctx(pt, renderer_mod, "C2")
    A = (wl.buffers[0], wl.buffers[1])
    fr = _inject()
    r.write_frame(fr)
    _setcam(r, *move(*A, forward=0.03))
    nan = float("nan")
    for args, code in [((0.5, 0.02, 0.9, False), -1), ((nan, 0.02, 0.9, False), -1), ((64, 0.0, 0.9, False), -1), ((64, -1.0, 0.9, False), -1),
                       ((64, nan, 0.9, False), -1), ((64, 0.02, 1.5, False), -1), ((64, 0.02, -1.5, False), -1), ((64, 0.02, nan, False), -1)]:
        with pytest.raises(renderer_mod.PtError) as e:
            r.reproject_frame(*args)
        assert e.value.code == code, args
        assert frames_equal(r.read_frame(), fr), args
    n = C.c_int64(7)
    assert r._L.pt_reproject_frame(r._h, 64.0, 0.02, 0.9, 2, C.byref(n)) == -1 and n.value == 0          # unknown flags
    assert r._L.pt_reproject_frame(None, 64.0, 0.02, 0.9, 0, C.byref(n)) == -1
    assert frames_equal(r.read_frame(), fr)
    p = wl.buffers[4].copy()
    p[10] = 1.0                                                 # DEBUG
    r.set_buffer(4, p)
    with pytest.raises(renderer_mod.PtError) as e:
        r.reproject_frame()
    assert e.value.code == -5
    p = wl.buffers[4].copy()
    p[2] = W / 2                                                # resolution no longer the image's
    r.set_buffer(4, p)
    with pytest.raises(renderer_mod.PtError) as e:
        r.reproject_frame()
    assert e.value.code == -1
    r.set_buffer(4, wl.buffers[4])
    r.set_buffer(14, wl.buffers[14])                            # a scene upload since the camera was recorded (even the same contents)
    with pytest.raises(renderer_mod.PtError) as e:
        r.reproject_frame()
    assert e.value.code == -1
    assert frames_equal(r.read_frame(), fr)
    r.write_frame(fr)
    r.set_texture(0, wl.sky)
    with pytest.raises(renderer_mod.PtError) as e:
        r.reproject_frame()
    assert e.value.code == -1
    assert frames_equal(r.read_frame(), fr)
    r.close()
    for kw in ({"shard_rank": 0, "shard_count": 2}, {"devices": [0], "first_shard": 0, "total_shards": 2}):
        r, wl = _ctx(pt, renderer_mod, "C2", **kw)
        r.render_batch(1, [pt.scenes.frame_seed(1)])
        before = r.read_frame()
        with pytest.raises(renderer_mod.PtError) as e:
            r.reproject_frame()
        assert e.value.code == -5, kw
        assert frames_equal(r.read_frame(), before)
        r.close()


def test_an_image_without_a_camera_is_left_alone(pt, renderer_mod):
    wl = pt.scenes.build("C2", W, H)
    r = renderer_mod.Renderer(W, H)
    fr = _inject()
    r.write_frame(fr)                                           # no Parameters yet: no camera
    r.load_workload(wl)
    assert r.reproject_frame() == 0 and frames_equal(r.read_frame(), fr)
    r.render_batch(1, [pt.scenes.frame_seed(1)])
    r.reset_frame()
    _setcam(r, *move(wl.buffers[0], wl.buffers[1], forward=0.03))
    assert r.reproject_frame() == 0 and not r.read_frame().any()
    r.render_batch(1, [pt.scenes.frame_seed(1)])
    r.next_image()
    assert r.reproject_frame() == 0 and not r.read_frame().any()
    r.close()


def test_reprojection_lowers_the_error_after_a_small_move(pt, renderer_mod):
    """C2: 16 frames at A, a small move, reproject and 2 frames beat reset and 2 frames against a 256-frame image at B"""
    r, wl = _ctx(pt, renderer_mod, "C2")
    A = (wl.buffers[0], wl.buffers[1])
    B = move(*A, forward=0.01, strafe=0.01, yaw=0.01)
    _setcam(r, *B)
    r.render_batch(1, [pt.scenes.frame_seed(5000 + f) for f in range(256)])
    ref = r.read_frame()
    _setcam(r, *A)
    r.reset_frame()
    r.render_batch(1, [pt.scenes.frame_seed(f) for f in range(1, 17)])
    _setcam(r, *B)
    kept = r.reproject_frame()
    r.render_batch(17, [pt.scenes.frame_seed(f) for f in range(17, 19)])
    reproj = r.read_frame()
    r.reset_frame()
    r.render_batch(1, [pt.scenes.frame_seed(f) for f in range(17, 19)])
    reset = r.read_frame()
    r.close()
    assert kept > 0.8 * W * H
    e_rp, e_rs = rmse(reproj, ref), rmse(reset, ref)
    assert e_rp < e_rs, (e_rp, e_rs)


def _adaptive_then_reproject(pt, renderer_mod, w, h, cols, mv, case):
    """C3 at w x h: two adaptive calls (every pixel 4 frames, then a partial one), a move, the reprojection; FRAME and the kept count against
    the model, then T through the selection of one more adaptive call (T has no reader: its active set is where FRAME's count grows)"""
    wl = pt.scenes.build("C3", w, h)
    r = renderer_mod.Renderer(w, h)
    r.load_workload(wl)
    A = (wl.buffers[0], wl.buffers[1])
    m = Model(cols)
    for first, n, rel, mn in ((1, 4, 0.0, 100), (5, 2, 0.5, 2)):
        got_n = r.render_adaptive(first, [pt.scenes.frame_seed(f) for f in range(first, first + n)], rel, 0.0, mn)
        assert got_n == int(m.adaptive(first, n, rel, 0.0, mn).sum())
    fr = r.read_frame()
    assert frames_equal(fr, m.F)
    rh = r.read_features()
    B = move(*A, **mv)
    _setcam(r, *B)
    rn = r.read_features()
    kept = r.reproject_frame(case["mh"], case["dt"], case["nt"], case["allm"])
    got = r.read_frame()
    want, wantT, wkept = _want(r, wl, rn, rh, fr, A, B, wl.buffers[2], T=m.T, **case)
    assert frames_equal(got, want), (w, h, mv, case, int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum()))
    assert kept == wkept and 0 < kept < w * h, (w, h, mv, case, kept, wkept)
    n = r.render_adaptive(7, [pt.scenes.frame_seed(7)], 0.3, 0.0, 3)
    act = r.read_frame()[..., 3] > got[..., 3]
    r.close()
    sel = select(wantT, 0.3, 0.0, 3, 0)
    assert np.array_equal(act, sel) and n == int(sel.sum()), (w, h, mv, case, n, int(sel.sum()), int((act != sel).sum()))
    if w * h > 100000:                                                      # the kept statistics decide: some kept pixels stay, some go
        assert 0 < int((sel & (want[..., 3] > 0)).sum()) < kept


def _uniform_cols(pt, renderer_mod, w, h, nf):
    wl = pt.scenes.build("C3", w, h)
    r = renderer_mod.Renderer(w, h)
    r.load_workload(wl)
    cols = []
    for f in range(1, nf + 1):                  # frame number 1 overwrites FRAME: the colour frame f adds (tests/test_gpu_adaptive_sizes.py)
        r.reset_frame()
        r.render(1, pt.scenes.frame_seed(f))
        cols.append(r.read_frame()[..., :3].copy())
    r.close()
    return cols


MOVES = [dict(forward=0.02, strafe=0.01), dict(yaw=0.03)]


@pytest.mark.parametrize("w,h", [(1920, 1080), (100, 7)])           # 100 x 7: a partial block of 64 columns, every block below its 16 rows
def test_full_size_and_edge_shapes_with_carried_statistics(pt, renderer_mod, w, h):
    cols = _uniform_cols(pt, renderer_mod, w, h, 6)
    for mv in MOVES:
        for case in CASES:
            _adaptive_then_reproject(pt, renderer_mod, w, h, cols, mv, case)
