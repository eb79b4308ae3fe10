"""GPU: reprojection across moved geometry (pt_motion_mark, pt_reproject_frame_moved; include/pt_motion.h) against the float32 model of
tests/_motion_model.py on the device's own feature records of M1 before and after the move; the identity to pt_reproject_frame when nothing
moved, a co-moving scene whose answer is known without any model, errors, contexts and later renders."""
import ctypes as C

import numpy as np
import pytest

import _motion_model as MM
from _reproject_model import cam_rot, frame_in, material_flags
from conftest import frames_equal
from test_gpu_reproject import CASES, _inject, _setcam, move

pytestmark = pytest.mark.gpu

W, H = 96, 54
GEOMETRY = (3, 7, 10, 11, 12, 13)
NO_MOUSE = np.array([-1.0e6, -1.0e6, 0.0], np.float32)


def _upload(r, wl):
    for b in GEOMETRY:
        r.set_buffer(b, wl.buffers[b])


def _inject_sized(w, h, seed=3):
    """_inject of tests/test_gpu_reproject.py at any size: counts 1 .. 99, a NaN, an inf and a patch of zero counts"""
    if (w, h) == (W, H):
        return _inject(seed)
    rs = np.random.RandomState(seed)
    cnt = rs.randint(1, 100, size=(h, w, 1)).astype(np.float32)
    fr = np.concatenate([rs.rand(h, w, 3).astype(np.float32) * cnt, cnt], -1)
    fr[h // 10, w // 13, 0] = np.nan
    fr[h // 6, w // 3, 1:3] = np.inf
    fr[h // 3: h // 3 + 3, w // 2: w // 2 + 4] = (1.0, 2.0, 3.0, 0.0)
    return fr


def _moments(w, h, seed=5):
    rs = np.random.RandomState(seed)
    n = rs.randint(0, 100, size=(h, w)).astype(np.float32)
    T = np.zeros((h, w, 4), np.float32)
    T[..., 0], T[..., 1], T[..., 2] = rs.rand(h, w) * n, rs.rand(h, w) * n * 2, n
    return T


def _want(r, wl_then, wl_now, rn, rh, fr, T, A, B, mouse_b, case, floor):
    cos = lambda x: r.debug_math("cos", x)      # noqa: E731  (the shader's own functions, as k_frame_setup calls them)
    sin = lambda x: r.debug_math("sin", x)      # noqa: E731
    fin_a = frame_in(wl_then.buffers[4], A[0], A[1], NO_MOUSE)
    fin_b = frame_in(wl_then.buffers[4], B[0], B[1], mouse_b)
    return MM.reproject_moved(rn, rh, fr, T, fin_a, fin_b, material_flags(wl_then.buffers[14]), cam_rot(A[1], cos, sin),
                              MM.tri_vertices(wl_now.buffers[3]), MM.tri_vertices(wl_then.buffers[3]), MM.ellipsoids(wl_now.buffers[7]),
                              MM.ellipsoids(wl_then.buffers[7]), case["mh"], case["dt"], case["nt"], case["allm"], floor)


def _one(r, wl_then, wl_now, fr, T, A, B, mouse_b, case, floor):
    """write FRAME and T under camera A in the scene `then`, mark, move to `now` and camera B, reproject: device against model"""
    w, h = wl_then.W, wl_then.H
    _upload(r, wl_then)
    _setcam(r, *A)
    r.set_buffer(2, NO_MOUSE)
    r.write_frame(fr)
    r.write_moments(T)
    rh = r.read_features()
    r.motion_mark()
    _upload(r, wl_now)
    _setcam(r, *B)
    r.set_buffer(2, mouse_b)
    rn = r.read_features()
    kept = r.reproject_frame_moved(case["mh"], case["dt"], case["nt"], case["allm"], floor)
    got, gotT = r.read_frame(), r.read_moments()
    want, wantT, wkept = _want(r, wl_then, wl_now, rn, rh, fr, T, A, B, mouse_b, case, floor)
    tag = (w, h, case, floor)
    assert frames_equal(got, want), (tag, int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum()))
    assert frames_equal(gotT, wantT), (tag, int((gotT.view(np.uint32) != wantT.view(np.uint32)).any(-1).sum()))
    assert kept == wkept and 0 < kept < w * h, (tag, kept, wkept)
    kind = MM.moved_point(rn, B[0], MM.tri_vertices(wl_now.buffers[3]), MM.tri_vertices(wl_then.buffers[3]), MM.ellipsoids(wl_now.buffers[7]),
                          MM.ellipsoids(wl_then.buffers[7]))[3].reshape(h, w)
    return kept, want, kind


def _m1(pt, step, w=W, h=H):
    return pt.scenes.m1_moving(step, w, h)


@pytest.mark.parametrize("steps", [(0, 1), (1, 3)])
def test_gpu_matches_the_model_on_m1(pt, renderer_mod, steps):
    wl0, wl1 = _m1(pt, steps[0]), _m1(pt, steps[1])
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl0)
    r.record_moments(True)
    A = (wl0.buffers[0], wl0.buffers[1])
    fr, T = _inject(), _moments(W, H)
    seen = set()
    for cam in (None, dict(forward=0.03, strafe=0.02, yaw=0.02)):
        B = A if cam is None else move(*A, **cam)
        for ci, case in enumerate(CASES):
            for floor in (0.0, 0.2):
                mouse_b = np.array([30.0, 17.0, 0.0], np.float32) if (cam is not None and ci == 0 and floor == 0.0) else NO_MOUSE
                kept, want, kind = _one(r, wl0, wl1, fr, T, A, B, mouse_b, case, floor)
                for k in (1, 2, 3):                              # pixels on unmoved primitives, moved triangles and the moved ellipsoid all keep history
                    assert ((kind == k) & (want[..., 3] > 0)).any(), (steps, cam, case, floor, k)
                seen.add(kept)
    assert len(seen) > 1
    r.close()


@pytest.mark.parametrize("w,h", [(1920, 1080), (100, 7)])           # 100 x 7: a partial block of 64 columns, every block below its 16 rows
def test_full_size_and_edge_shapes(pt, renderer_mod, w, h):
    wl0, wl1 = _m1(pt, 0, w, h), _m1(pt, 2, w, h)
    r = renderer_mod.Renderer(w, h)
    r.load_workload(wl0)
    r.record_moments(True)
    A = (wl0.buffers[0], wl0.buffers[1])
    B = move(*A, forward=0.02, strafe=0.01, yaw=0.01)
    _one(r, wl0, wl1, _inject_sized(w, h), _moments(w, h), A, B, NO_MOUSE, CASES[0], 0.0)
    _one(r, wl0, wl1, _inject_sized(w, h), _moments(w, h), A, A, NO_MOUSE, CASES[1], 0.2)
    r.close()


@pytest.mark.parametrize("floor", [0.0, 0.2])
def test_identical_geometry_is_pt_reproject_frame(pt, renderer_mod, floor):
    """the geometry buffers uploaded again byte for byte and the camera moved: pt_reproject_frame (pt_reproject_frame_demod) on a twin context
    that uploaded nothing, bit for bit"""
    out = []
    for moved in (True, False):
        wl = pt.scenes.build("C3", W, H)
        r = renderer_mod.Renderer(W, H)
        r.load_workload(wl)
        r.record_moments(True)
        A = (wl.buffers[0], wl.buffers[1])
        r.write_frame(_inject())
        r.write_moments(_moments(W, H))
        if moved:
            r.motion_mark()
            _upload(r, wl)
        _setcam(r, *move(*A, forward=0.03, strafe=0.02, yaw=0.02))
        if moved:
            kept = r.reproject_frame_moved(albedo_floor=floor)
        else:
            kept = r.reproject_frame(albedo_floor=floor if floor else None)
        out.append((kept, r.read_frame(), r.read_moments()))
        r.close()
    (k1, f1, t1), (k0, f0, t0) = out
    assert 0 < k0 < W * H and k1 == k0
    assert frames_equal(f1, f0) and frames_equal(t1, t0)


def _c2_shifted(pt, d):
    """C2 with every vertex and the camera translated by d"""
    S = pt.scenes
    sc = S._new_scene()
    S._cornell_materials(sc)
    o = S.Obj()
    S._cornell_room(o)
    lines = []
    for ln in o.lines:
        if ln.startswith("v "):
            x, y, z = (float(v) for v in ln.split()[1:])
            ln = "v %.9g %.9g %.9g" % (x + d[0], y + d[1], z + d[2])
        lines.append(ln)
    o.lines = lines
    sc.addObjectText(o.text(), 0, parentDirectory="")
    cam = tuple(float(c) + float(v) for c, v in zip(S.CORNELL_CAM, d))
    return S._finish("C2", sc, W, H, cam, S.CORNELL_ROT, (0, 0, 0), 8, 8)


CO_MOVE = (0.25, 0.125, -0.5)       # chosen on the CPU: the oracle's rayScene gives 13 of 5184 pixels (0.25 %) another hit code in the translated C2; the bound is 2 %


def test_co_moving_scene_maps_every_pixel_onto_itself(pt, renderer_mod):
    """All of C2 and the camera translated by one vector: every ray meets the same surface point as before, so — whatever the model says — the
    result of a pixel whose hit code is unchanged, on a material that is not view-dependent, with a valid FRAME, is its own FRAME (the history cap
    is out of reach here).  Rays pass through pixel centres, so s = p holds with half a pixel of margin."""
    wl0, wl1 = _c2_shifted(pt, (0.0, 0.0, 0.0)), _c2_shifted(pt, CO_MOVE)
    assert not material_flags(wl0.buffers[14]).any()
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl0)
    fr = _inject()
    r.write_frame(fr)
    rh = r.read_features()
    r.motion_mark()
    _upload(r, wl1)
    _setcam(r, wl1.buffers[0], wl1.buffers[1])
    rn = r.read_features()
    kept = r.reproject_frame_moved(max_history=1.0e9)
    got = r.read_frame()
    r.close()
    code_n, code_h = (np.ascontiguousarray(f[..., 7]).view(np.int32) for f in (rn, rh))
    differ = code_n != code_h
    print(f"co-moving C2: {int(differ.sum())} of {W * H} pixels change their hit code, kept {kept}")
    assert differ.mean() < 0.02
    valid = (fr[..., 3] > 0) & np.isfinite(fr[..., :3]).all(-1)
    check = ~differ & (code_n != -1) & valid
    assert check.sum() > 0.9 * W * H
    assert np.array_equal(got[check].view(np.uint32), fr[check].view(np.uint32)), int((got[check].view(np.uint32) != fr[check].view(np.uint32)).any(-1).sum())
    assert not got[~valid & ~differ].any()


def test_errors_leave_frame_unchanged(pt, renderer_mod):
    wl0, wl1 = _m1(pt, 0), _m1(pt, 1)
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl0)
    fr = _inject()
    r.write_frame(fr)

    def refused(code, call=None, **kw):
        with pytest.raises(renderer_mod.PtError) as e:
            (call or r.reproject_frame_moved)(**kw)
        assert e.value.code == code, (code, e.value.code, kw)
        assert frames_equal(r.read_frame(), fr)

    refused(-1)                                                 # no mark
    r.motion_mark()
    _upload(r, wl1)
    nan = float("nan")
    for kw in (dict(max_history=0.5), dict(depth_tol=0.0), dict(normal_tol=1.5), dict(albedo_floor=-0.1), dict(albedo_floor=nan),
               dict(albedo_floor=float("inf")), dict(max_history=nan)):
        refused(-1, **kw)
    n = C.c_int64(7)
    assert r._L.pt_reproject_frame_moved(r._h, 64.0, 0.02, 0.9, 2, 0.0, C.byref(n)) == -1 and n.value == 0      # unknown flags
    assert r._L.pt_reproject_frame_moved(None, 64.0, 0.02, 0.9, 0, 0.0, C.byref(n)) == -1
    assert r._L.pt_motion_mark(None) == -1
    refused(-1, call=r.reproject_frame)                         # pt_reproject_frame still refuses after a geometry upload
    p = wl0.buffers[4].copy()
    p[10] = 1.0                                                 # DEBUG
    r.set_buffer(4, p)
    refused(-5)
    r.set_buffer(4, wl0.buffers[4])
    assert r.reproject_frame_moved() > 0                        # the errors above left the mark in place
    fr = r.read_frame()
    refused(-1)                                                 # ... and it is spent now
    r.motion_mark()                                             # the call recorded the camera anew, in the scene as it is now
    r.motion_mark()                                             # a second mark replaces the first
    assert r.reproject_frame_moved() > 0                        # (nothing moved since)
    r.close()


def _marked(pt, renderer_mod, **kw):
    wl0, wl1 = _m1(pt, 0), _m1(pt, 1)
    r = renderer_mod.Renderer(W, H, **kw)
    r.load_workload(wl0)
    r.render_batch(1, [pt.scenes.frame_seed(f) for f in (1, 2)])
    return r, wl0, wl1


@pytest.mark.parametrize("between", ["render", "write_frame", "reset_frame", "next_image", "materials", "implicits", "texture", "mark_after_upload"])
def test_a_stale_mark_is_refused(pt, renderer_mod, between):
    r, wl0, wl1 = _marked(pt, renderer_mod)
    if between != "mark_after_upload":
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
    before = r.read_frame()
    with pytest.raises(renderer_mod.PtError) as e:
        (r.motion_mark if between == "mark_after_upload" else r.reproject_frame_moved)()
    assert e.value.code == -1
    assert frames_equal(r.read_frame(), before)
    r.close()


def test_part_image_contexts_and_debug_are_unsupported(pt, renderer_mod):
    for kw in ({"shard_rank": 0, "shard_count": 2}, {"devices": [0], "first_shard": 0, "total_shards": 2}):
        r, wl0, wl1 = _marked(pt, renderer_mod, **kw)
        before = r.read_frame()
        for call in (r.motion_mark, r.reproject_frame_moved):
            with pytest.raises(renderer_mod.PtError) as e:
                call()
            assert e.value.code == -5, kw
        assert frames_equal(r.read_frame(), before)
        r.close()
    wl = _m1(pt, 0)
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl.with_params(DEBUG=1.0))
    r.render_batch(1, [pt.scenes.frame_seed(1)])
    before = r.read_frame()
    with pytest.raises(renderer_mod.PtError) as e:
        r.motion_mark()                                         # the image was rendered with DEBUG != 0
    assert e.value.code == -5 and frames_equal(r.read_frame(), before)
    r.close()


def _sequence(pt, renderer_mod, **kw):
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 9)]
    r, wl0, wl1 = _marked(pt, renderer_mod, **kw)
    r.record_moments(True)
    r.reset_frame()
    r.render_batch(2, seeds[:4])
    r.motion_mark()
    _upload(r, wl1)
    _setcam(r, *move(wl0.buffers[0], wl0.buffers[1], forward=0.02, yaw=0.01))
    kept = r.reproject_frame_moved(max_history=3.0, albedo_floor=0.2)
    mid, midT = r.read_frame(), r.read_moments()
    r.render_batch(6, seeds[4:7])
    out = r.read_frame()
    r.close()
    return kept, mid, midT, out


def test_multi_stream_context_equals_one_stream(pt, renderer_mod):
    k0, m0, t0, f0 = _sequence(pt, renderer_mod)
    assert 0 < k0 < W * H and t0[..., 2].max() == 3.0
    for kw in ({"devices": [0, 0]}, {"devices": [0]}):
        k1, m1, t1, f1 = _sequence(pt, renderer_mod, **kw)
        assert k1 == k0, kw
        assert frames_equal(m1, m0) and frames_equal(t1, t0) and frames_equal(f1, f0), kw


def test_later_renders_equal_renders_on_the_written_result(pt, renderer_mod):
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 9)]
    wl0, wl1 = _m1(pt, 0), _m1(pt, 1)
    B = move(wl0.buffers[0], wl0.buffers[1], forward=0.02, strafe=-0.02, yaw=-0.02)
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl0)
    r.render_batch(1, seeds[:4])
    r.motion_mark()
    _upload(r, wl1)
    _setcam(r, *B)
    assert r.reproject_frame_moved() > 0
    mid = r.read_frame()
    r.render_batch(5, seeds[4:8])
    got = r.read_frame()
    r.close()
    r2 = renderer_mod.Renderer(W, H)
    r2.load_workload(wl1)
    _setcam(r2, *B)
    r2.write_frame(mid)
    r2.render_batch(5, seeds[4:8])
    want = r2.read_frame()
    r2.close()
    assert frames_equal(got, want)
