"""GPU: reprojection across moved geometry with bilinear taps (pt_reproject_frame_moved_bilinear; include/pt_motion_bilinear.h) held to the float32
model of tests/_motion_bilinear_model.py bit for bit in FRAME, T and both counts, on the device's own feature records of M1 before and after the
move; then what needs no model: nothing moved against pt_reproject_frame_bilinear and pt_reproject_frame_moved on a twin context, the kept set,
contexts, later renders, every refusal with FRAME, T and the mark unchanged, the image without a camera."""
import ctypes as C

import numpy as np
import pytest

import _motion_model as MM
from _motion_bilinear_model import reproject_moved_bilinear as model
from _reproject_model import cam_rot, frame_in, material_flags
from conftest import frames_equal
from test_gpu_motion import NO_MOUSE, _inject_sized, _moments, _upload
from test_gpu_reproject import _setcam, move

pytestmark = pytest.mark.gpu

W, H = 96, 54
SIZES = [(96, 54), (100, 7), (130, 33)]     # M1's default; a partial block in x and y, one block row; three block columns, a block row of one row
POSES = [(0, 0.25), (1, 1.5), (0, 1)]
SHIFT = np.array([0.011, 0.0, 0.017], np.float32)
SCENES = {"M1-plain": (False, 0.0), "M1-textured": (True, 0.05)}
# the blended pixels every run must at least have on moved triangles and on the moved ellipsoid (which M1's camera does not see at the two thin
# sizes).  The model on the oracle's records gives 40-46 of 45-50 at 100 x 7, 320-364 at 130 x 33 and 255-314 / 100-110 at 96 x 54, with the
# injected frames of _injected as with the clean ones.
AT_LEAST = {(100, 7): (30, 0), (130, 33): (200, 0), (96, 54): (200, 80)}


def _m1(pt, step, w=W, h=H, textured=True):
    return pt.scenes.m1_moving(step, w, h, textured=textured)


def _clean(w, h, seed=3):
    """a FRAME of random means and counts 1 .. 99, every pixel valid"""
    rs = np.random.RandomState(seed)
    cnt = rs.randint(1, 100, size=(h, w, 1)).astype(np.float32)
    return np.concatenate([rs.rand(h, w, 3).astype(np.float32) * cnt, cnt], -1)


def _injected(w, h):
    """_inject_sized of tests/test_gpu_motion.py: counts 1 .. 99, a NaN, an inf and a patch of zero counts.  At 100 x 7 its patch (columns 50-53)
    covers a third of the 45-50 pixels on moved triangles (columns 45-54), so it is put beside them, at columns 60-63"""
    fr = _inject_sized(w, h)
    if (w, h) == (100, 7):
        fr[2:5, 50:54] = _clean(w, h)[2:5, 50:54]               # (the same seed: what _inject_sized had there)
        fr[2:5, 60:64] = (1.0, 2.0, 3.0, 0.0)
    return fr


def _geo(wl_then, wl_now):
    return (MM.tri_vertices(wl_now.buffers[3]), MM.tri_vertices(wl_then.buffers[3]), MM.ellipsoids(wl_now.buffers[7]), MM.ellipsoids(wl_then.buffers[7]))


def _bits(a, b):
    return int((np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)).any(-1).sum())


def _one(r, wl_then, wl_now, fr, T, A, B, mouse_b, rule, floor):
    """write FRAME (and T) under camera A in the scene `then`, mark, move to `now` and camera B, call: device against model.  Returns the blended
    pixels on moved triangles and on moved ellipsoids."""
    w, h = wl_then.W, wl_then.H
    _upload(r, wl_then)
    _setcam(r, *A)
    r.set_buffer(2, NO_MOUSE)
    r.write_frame(fr)
    if T is not None:
        r.write_moments(T)
    rh = r.read_features()
    r.motion_mark()
    _upload(r, wl_now)
    _setcam(r, *B)
    r.set_buffer(2, mouse_b)
    rn = r.read_features()
    kept, blended = r.reproject_frame_moved_bilinear(rule["mh"], rule["dt"], rule["nt"], rule["snap"], rule["allm"], floor)
    got, gotT = r.read_frame(), r.read_moments()
    cos = lambda x: r.debug_math("cos", x)      # noqa: E731  (the shader's own functions, as k_frame_setup calls them)
    sin = lambda x: r.debug_math("sin", x)      # noqa: E731
    fin_a = frame_in(wl_then.buffers[4], A[0], A[1], NO_MOUSE)
    fin_b = frame_in(wl_then.buffers[4], B[0], B[1], mouse_b)
    geo = _geo(wl_then, wl_now)
    want, wantT, wkept, wblended, d = model(rn, rh, fr, T, fin_a, fin_b, material_flags(wl_then.buffers[14]), cam_rot(A[1], cos, sin), *geo,
                                            rule["mh"], rule["dt"], rule["nt"], rule["snap"], rule["allm"], floor, detail=True)
    kind = MM.moved_point(rn, B[0], *geo)[3].reshape(h, w)
    on_tri, on_el = int(((kind == 2) & (d["taps"] >= 2)).sum()), int(((kind == 3) & (d["taps"] >= 2)).sum())
    tag = (w, h, rule, floor, T is not None)
    print(f"{w}x{h} floor {floor} T={T is not None} snap {rule['snap']}: kept {kept} / {wkept}, blended {blended} / {wblended} of {w * h}; blended on moved "
          f"triangles {on_tri} of {int((kind == 2).sum())}, on the moved ellipsoid {on_el} of {int((kind == 3).sum())}")
    assert frames_equal(got, want), (tag, _bits(got, want))
    if T is not None:
        assert frames_equal(gotT, wantT), (tag, _bits(gotT, wantT))
    else:
        assert not gotT.any(), tag
    assert (kept, blended) == (wkept, wblended) and 0 < blended <= kept <= w * h, (tag, kept, wkept, blended, wblended)
    return on_tri, on_el


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("scene", list(SCENES))
def test_gpu_matches_the_model(pt, renderer_mod, scene, w, h):
    textured, floor = SCENES[scene]
    r = renderer_mod.Renderer(w, h)
    r.load_workload(_m1(pt, 0, w, h, textured))
    mouse = np.array([w * 0.3, h * 0.6, 0.0], np.float32)
    # (T, overlay, injected NaN / inf / zero-count cells, rule): T is allocated by the first pt_write_moments, so the runs without it come first
    variants = [(False, NO_MOUSE, False, dict(mh=64.0, dt=0.02, nt=0.9, snap=1.0 / 64, allm=False)),
                (True, mouse, True, dict(mh=64.0, dt=0.02, nt=0.9, snap=1.0 / 64, allm=False)),
                (True, NO_MOUSE, False, dict(mh=10.0, dt=0.05, nt=0.5, snap=0.0, allm=True))]
    need_tri, need_el = AT_LEAST[(w, h)]
    for with_t, mouse_b, bad, rule in variants:
        fr = _injected(w, h) if bad else _clean(w, h)
        T = _moments(w, h) if with_t else None
        for s0, s1 in POSES:
            wl0, wl1 = _m1(pt, s0, w, h, textured), _m1(pt, s1, w, h, textured)
            A = (np.asarray(wl0.buffers[0], np.float32)[:3].copy(), np.asarray(wl0.buffers[1], np.float32)[:3].copy())
            for B in (A, ((A[0] + SHIFT).astype(np.float32), A[1])):
                on_tri, on_el = _one(r, wl0, wl1, fr, T, A, B, mouse_b, rule, floor)
                assert on_tri >= need_tri and on_el >= need_el, (scene, w, h, s0, s1, bad, on_tri, on_el)
    r.close()


def _twins(pt, renderer_mod, w, h, step=0):
    wl = _m1(pt, step, w, h)
    out = []
    for _ in range(2):
        r = renderer_mod.Renderer(w, h)
        r.load_workload(wl)
        out.append(r)
    return out[0], out[1], wl


@pytest.mark.parametrize("w,h", SIZES)
def test_nothing_moved_equals_the_bilinear_and_the_moved_call_on_a_twin(pt, renderer_mod, w, h):
    r, twin, wl = _twins(pt, renderer_mod, w, h)
    A = (wl.buffers[0], wl.buffers[1])
    B = ((np.asarray(A[0], np.float32)[:3] + SHIFT).astype(np.float32), A[1])
    fr, T = _inject_sized(w, h), _moments(w, h)
    for floor in (0.0, 0.05):
        # the geometry uploaded again byte for byte and the camera moved: pt_reproject_frame_bilinear on a twin that uploaded nothing
        for x in (r, twin):
            _setcam(x, *A)
            x.write_frame(fr)
            x.write_moments(T)
        r.motion_mark()
        _upload(r, wl)
        for x in (r, twin):
            _setcam(x, *B)
        kept, blended = r.reproject_frame_moved_bilinear(albedo_floor=floor)
        wkept, wblended = twin.reproject_frame_bilinear(albedo_floor=floor)
        assert (kept, blended) == (wkept, wblended) and 0 < blended <= kept < w * h, (w, h, floor, kept, wkept, blended, wblended)
        assert frames_equal(r.read_frame(), twin.read_frame()) and frames_equal(r.read_moments(), twin.read_moments()), (w, h, floor)
        # the camera unchanged as well: pt_reproject_frame_moved on the twin, and no pixel blended
        for x in (r, twin):
            _setcam(x, *A)
            x.write_frame(fr)
            x.write_moments(T)
            x.motion_mark()
            _upload(x, wl)
        kept, blended = r.reproject_frame_moved_bilinear(albedo_floor=floor)
        wkept = twin.reproject_frame_moved(albedo_floor=floor)
        assert kept == wkept and blended == 0 and 0 < kept < w * h, (w, h, floor, kept, wkept, blended)
        assert frames_equal(r.read_frame(), twin.read_frame()) and frames_equal(r.read_moments(), twin.read_moments()), (w, h, floor)
    r.close()
    twin.close()


def test_keeps_every_pixel_the_nearest_moved_call_keeps(pt, renderer_mod):
    r, twin, wl0 = _twins(pt, renderer_mod, W, H)
    A = (wl0.buffers[0], wl0.buffers[1])
    fr, T = _inject_sized(W, H), _moments(W, H)
    for (s0, s1), cam in zip(POSES, (None, dict(forward=0.03, strafe=0.02, yaw=0.02), dict(forward=0.004, strafe=0.02))):
        wl_then, wl_now = _m1(pt, s0), _m1(pt, s1)
        for x in (r, twin):
            _upload(x, wl_then)
            _setcam(x, *A)
            x.write_frame(fr)
            x.write_moments(T)
            x.motion_mark()
            _upload(x, wl_now)
            if cam:
                _setcam(x, *move(*A, **cam))
        kept, blended = r.reproject_frame_moved_bilinear(albedo_floor=0.05)
        near = twin.reproject_frame_moved(albedo_floor=0.05)
        got, want = r.read_frame(), twin.read_frame()
        print(f"M1 {s0} -> {s1}, camera {cam}: nearest keeps {near}, bilinear {kept} (blended {blended}) of {W * H}")
        assert kept >= near > 0 and 0 < blended <= kept, (s0, s1, kept, near, blended)
        assert (got[..., 3] > 0)[want[..., 3] > 0].all(), (s0, s1)
        assert kept == int((got[..., 3] > 0).sum())
    r.close()
    twin.close()


def _sequence(pt, renderer_mod, **kw):
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 9)]
    wl0, wl1 = _m1(pt, 0), _m1(pt, 0.25)
    r = renderer_mod.Renderer(W, H, **kw)
    r.load_workload(wl0)
    r.record_moments(True)
    r.render_batch(2, seeds[:4])
    r.motion_mark()
    _upload(r, wl1)
    _setcam(r, *move(wl0.buffers[0], wl0.buffers[1], forward=0.02, yaw=0.01))
    kept, blended = r.reproject_frame_moved_bilinear(max_history=3.0, albedo_floor=0.2)
    mid, midT = r.read_frame(), r.read_moments()
    r.render_batch(6, seeds[4:7])
    out = r.read_frame()
    r.close()
    return kept, blended, mid, midT, out


def test_multi_stream_context_equals_one_stream(pt, renderer_mod):
    k0, b0, m0, t0, f0 = _sequence(pt, renderer_mod)
    assert 0 < b0 <= k0 < W * H and t0[..., 2].max() == 3.0
    for kw in ({"devices": [0, 0]}, {"devices": [0]}):
        k1, b1, m1, t1, f1 = _sequence(pt, renderer_mod, **kw)
        assert (k1, b1) == (k0, b0), kw
        assert frames_equal(m1, m0) and frames_equal(t1, t0) and frames_equal(f1, f0), kw


def test_later_renders_equal_renders_on_the_written_result(pt, renderer_mod):
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 9)]
    wl0, wl1 = _m1(pt, 0), _m1(pt, 0.25)
    B = move(wl0.buffers[0], wl0.buffers[1], forward=0.02, strafe=-0.02, yaw=-0.02)
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl0)
    r.record_moments(True)
    r.render_batch(1, seeds[:4])
    r.motion_mark()
    _upload(r, wl1)
    _setcam(r, *B)
    kept, blended = r.reproject_frame_moved_bilinear()
    assert 0 < blended <= kept < W * H
    mid, midT = r.read_frame(), r.read_moments()
    r.render_batch(5, seeds[4:8])
    got, gotT = r.read_frame(), r.read_moments()
    r.close()
    r2 = renderer_mod.Renderer(W, H)
    r2.load_workload(wl1)
    r2.record_moments(True)
    _setcam(r2, *B)
    r2.write_frame(mid)
    r2.write_moments(midT)
    r2.render_batch(5, seeds[4:8])
    want, wantT = r2.read_frame(), r2.read_moments()
    r2.close()
    assert frames_equal(got, want) and frames_equal(gotT, wantT)


NAME = "pt_reproject_frame_moved_bilinear: "


def test_argument_errors_leave_frame_t_and_the_mark(pt, renderer_mod):
    Rule = renderer_mod.ReprojectBilinearRule
    wl0, wl1 = _m1(pt, 0), _m1(pt, 0.25)
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl0)
    fr, T = _inject_sized(W, H), _moments(W, H)
    r.write_frame(fr)
    r.write_moments(T)
    nan, inf = float("nan"), float("inf")

    def same():
        return frames_equal(r.read_frame(), fr) and frames_equal(r.read_moments(), T)

    def raw(rule, ctx=True):
        n, nb = C.c_int64(7), C.c_int64(7)
        rc = r._L.pt_reproject_frame_moved_bilinear(r._h if ctx else None, C.byref(rule) if rule is not None else None, C.byref(n), C.byref(nb))
        return rc, n.value, nb.value, r._L.pt_last_error().decode()

    good = dict(max_history=64.0, depth_tol=0.02, normal_tol=0.9, snap=1.0 / 64, albedo_floor=0.0, flags=0)
    rc, n, nb, msg = raw(Rule(**good))                          # no mark
    assert (rc, n, nb) == (-1, 0, 0) and msg.startswith(NAME + "no mark") and same()
    r.motion_mark()
    _upload(r, wl1)
    bad = [(dict(max_history=0.5), "max_history"), (dict(max_history=nan), "max_history"), (dict(depth_tol=0.0), "depth_tol"), (dict(depth_tol=-1.0), "depth_tol"),
           (dict(depth_tol=nan), "depth_tol"), (dict(normal_tol=1.5), "normal_tol"), (dict(normal_tol=-1.5), "normal_tol"), (dict(normal_tol=nan), "normal_tol"),
           (dict(flags=2), "unknown flags"), (dict(snap=-0.01), "rule.snap must be in [0, 0.5)"), (dict(snap=0.5), "rule.snap"), (dict(snap=nan), "rule.snap"),
           (dict(snap=inf), "rule.snap"), (dict(albedo_floor=-0.1), "rule.albedo_floor"), (dict(albedo_floor=nan), "rule.albedo_floor"),
           (dict(albedo_floor=inf), "rule.albedo_floor")]
    for kw, what in bad:
        rc, n, nb, msg = raw(Rule(**{**good, **kw}))
        assert (rc, n, nb) == (-1, 0, 0) and msg.startswith(NAME + what), (kw, msg)
        assert same(), kw
    rc, n, nb, msg = raw(None)
    assert (rc, n, nb) == (-1, 0, 0) and msg == NAME + "null argument" and same()
    assert raw(Rule(**good), ctx=False)[:3] == (-1, 0, 0) and same()
    assert r._L.pt_reproject_frame_moved_bilinear(r._h, None, None, None) == -1
    with pytest.raises(renderer_mod.PtError) as e:
        r.reproject_frame_moved_bilinear(snap=0.75)
    assert e.value.code == -1 and NAME in str(e.value)
    p = wl0.buffers[4].copy()
    p[10] = 1.0                                                 # DEBUG
    r.set_buffer(4, p)
    rc, n, nb, msg = raw(Rule(**good))
    assert (rc, n, nb) == (-5, 0, 0) and msg.startswith(NAME) and same()
    p = wl0.buffers[4].copy()
    p[2] = W / 2                                                # resolution no longer the image's
    r.set_buffer(4, p)
    assert raw(Rule(**good))[:3] == (-1, 0, 0) and same()         # (this text names the Parameters, not the call, for every call)
    r.set_buffer(4, wl0.buffers[4])
    with pytest.raises(renderer_mod.PtError):
        r.reproject_frame()                                     # pt_reproject_frame still refuses after a geometry upload
    assert same()
    # every refusal above left the mark in place: the same mark serves a good call, with null count pointers too, and is spent by it
    assert r._L.pt_reproject_frame_moved_bilinear(r._h, C.byref(Rule(**good)), None, None) == 0 and not same()
    fr = r.read_frame()
    rc, n, nb, msg = raw(Rule(**good))
    assert (rc, n, nb) == (-1, 0, 0) and msg.startswith(NAME + "no mark") and frames_equal(r.read_frame(), fr)
    r.motion_mark()                                             # the call recorded the camera anew, in the scene as it is now
    kept, blended = r.reproject_frame_moved_bilinear()          # (nothing moved since, the camera unchanged)
    assert kept > 0 and blended == 0
    r.close()


def _marked(pt, renderer_mod, **kw):
    wl0, wl1 = _m1(pt, 0), _m1(pt, 0.25)
    r = renderer_mod.Renderer(W, H, **kw)
    r.load_workload(wl0)
    if not kw:
        r.record_moments(True)
    r.render_batch(1, [pt.scenes.frame_seed(f) for f in (1, 2)])
    return r, wl0, wl1


@pytest.mark.parametrize("between", ["render", "write_frame", "reset_frame", "next_image", "materials", "implicits", "texture"])
def test_a_stale_mark_is_refused(pt, renderer_mod, between):
    r, wl0, wl1 = _marked(pt, renderer_mod)
    r.motion_mark()
    _upload(r, wl1)
    if between == "render":
        r.render_batch(3, [pt.scenes.frame_seed(3)])
    elif between == "write_frame":
        r.write_frame(r.read_frame())
    elif between == "reset_frame":
        r.reset_frame()
    elif between == "next_image":
        r.next_image()
    elif between == "materials":
        r.set_buffer(14, wl0.buffers[14])
    elif between == "implicits":
        r.set_buffer(5, wl0.buffers[5])
    elif between == "texture":
        r.set_texture(1, wl0.textures[1])
    before, beforeT = r.read_frame(), r.read_moments()
    with pytest.raises(renderer_mod.PtError) as e:
        r.reproject_frame_moved_bilinear()
    assert e.value.code == -1 and NAME in str(e.value)
    assert frames_equal(r.read_frame(), before) and frames_equal(r.read_moments(), beforeT)
    r.close()


def test_another_images_mark_is_refused(pt, renderer_mod):
    r, wl0, wl1 = _marked(pt, renderer_mod)
    r.motion_mark()
    r.next_image()
    r.render_batch(1, [pt.scenes.frame_seed(1)])                # the new image has a camera of its own; the mark belongs to the other one
    _upload(r, wl1)
    before = r.read_frame()
    with pytest.raises(renderer_mod.PtError) as e:
        r.reproject_frame_moved_bilinear()
    assert e.value.code == -1 and NAME in str(e.value) and frames_equal(r.read_frame(), before)
    r.close()


def test_part_image_contexts_are_unsupported(pt, renderer_mod):
    for kw in ({"shard_rank": 0, "shard_count": 2}, {"devices": [0], "first_shard": 0, "total_shards": 2}):
        r, wl0, wl1 = _marked(pt, renderer_mod, **kw)
        before = r.read_frame()
        with pytest.raises(renderer_mod.PtError) as e:
            r.reproject_frame_moved_bilinear()
        assert e.value.code == -5 and NAME.rstrip(": ") in str(e.value), kw
        assert frames_equal(r.read_frame(), before)
        r.close()


def test_an_image_without_a_camera_is_left_alone(pt, renderer_mod):
    """no camera and no mark: PT_OK with both counts 0 (with a mark taken before the camera went: test_a_stale_mark_is_refused)"""
    wl = _m1(pt, 0)
    r = renderer_mod.Renderer(W, H)
    fr = _inject_sized(W, H)
    r.write_frame(fr)                                           # no Parameters yet: no camera
    r.load_workload(wl)
    assert r.reproject_frame_moved_bilinear() == (0, 0) and frames_equal(r.read_frame(), fr)
    r.render_batch(1, [pt.scenes.frame_seed(1)])
    r.reset_frame()
    _setcam(r, *move(wl.buffers[0], wl.buffers[1], forward=0.03))
    assert r.reproject_frame_moved_bilinear() == (0, 0) and not r.read_frame().any()
    r.close()
