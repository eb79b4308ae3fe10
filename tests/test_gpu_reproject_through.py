"""GPU: reprojection of mirror and glass pixels through their seen-through chains (pt_reproject_frame_through; include/pt_reproject_through.h)
against the float32 model of tests/_reproject_through_model.py, bit for bit in FRAME, T and both counts, on the records of real scenes and
FRAMEs and Ts injected through pt_write_frame / pt_write_moments; the degenerate rules, the unchanged camera, contexts, later renders, the
hold, every error, the no-op, and its effect on noise."""
import ctypes as C

import numpy as np
import pytest

from _reproject_model import cam_rot, frame_in, material_flags
from _reproject_through_model import reproject_through as model
from conftest import frames_equal
from test_gpu_reproject import _setcam, move

pytestmark = pytest.mark.gpu

W, H = 96, 54
REFLECT, TRANSMIT = 1, 2
CHAINS = dict(max_depth=4, min_weight=0.5, lobes=REFLECT | TRANSMIT, key=True)
SMALL = dict(forward=0.01, strafe=0.005, yaw=0.005)
NO_MOUSE = np.array([-1.0e6, -1.0e6, 0.0], np.float32)


def _ctx(pt, renderer_mod, name="C3", w=W, h=H, **kw):
    wl = pt.scenes.build(name, w, h)
    r = renderer_mod.Renderer(w, h, **kw)
    r.load_workload(wl)
    return r, wl


def _inject(w, h, seed=3):
    """FRAME and T with a NaN, infs, zero-count cells and counts on both sides of the caps the tests use"""
    rs = np.random.RandomState(seed)
    cnt = rs.randint(1, 100, size=(h, w, 1)).astype(np.float32)
    fr = np.concatenate([rs.rand(h, w, 3).astype(np.float32) * cnt, cnt], -1)
    n = rs.randint(1, 100, size=(h, w)).astype(np.float32)
    T = np.stack([rs.rand(h, w).astype(np.float32) * n, rs.rand(h, w).astype(np.float32) * n, n, np.zeros((h, w), np.float32)], -1)
    fr[h // 3, w // 5, 0] = np.nan
    fr[h // 2, w // 3, 1:3] = np.inf
    fr[h // 2:h // 2 + 2, w // 2:w // 2 + 3] = (1.0, 2.0, 3.0, 0.0)
    fr[::5, 2::7, 3] = 0.0                                          # zero-count cells all over: a nearest candidate without history
    T[h // 3, (w // 5 + 1) % w, 0] = np.inf
    T[::4, 1::6, 2] = 0.0
    return fr, T


def _differ(a, b):
    return int((np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)).any(-1).sum())


def _records(r, thru):
    return r.read_features(), r.read_features_through(thru), r.read_through_rays(thru)


def _want(r, wl, recs_n, recs_h, fr, T, A, B, mouse_b, rule):
    cos = lambda x: r.debug_math("cos", x)      # noqa: E731  (the shader's own functions, as k_frame_setup calls them)
    sin = lambda x: r.debug_math("sin", x)      # noqa: E731
    fin_a = frame_in(wl.buffers[4], A[0], A[1], wl.buffers[2])
    fin_b = frame_in(wl.buffers[4], B[0], B[1], mouse_b)
    (rn, sn, yn), (rh, sh, yh) = recs_n, recs_h
    return model(rn, rh, sn, sh, yn, yh, fr, T, fin_a, fin_b, material_flags(wl.buffers[14]), cam_rot(A[1], cos, sin), rule["mh"], rule["dt"], rule["nt"],
                 rule["tol"], rule["radius"], rule["allm"])


def _rule(r, rule):
    return r.reproject_through_rule(rule["mh"], rule["dt"], rule["nt"], rule["tol"], rule["radius"], rule["allm"])


RULES = [dict(mh=10.0 if allm else 64.0, dt=0.05 if allm else 0.02, nt=0.5 if allm else 0.9, tol=tol, radius=radius, allm=allm)
         for radius in (0, 2, 4) for tol in (0.05, 0.02) for allm in (False, True)]
# the model must keep this many chain pixels (and this many at a source other than the guess) under radius 2, point_tol 0.05, without
# PT_REPROJECT_ALL_MATERIALS, so that the comparison cannot pass on an empty search (a float64 sketch on the oracle: 579 and 361 of 645; 551)
FLOORS = {("C3", 96, 54): (400, 200), ("C3", 130, 35): (300, 0)}


@pytest.mark.parametrize("scene,w,h", [("C3", 96, 54), ("C3", 130, 35), ("C3", 100, 7), ("C3", 5, 3), ("C6", 96, 54), ("T1", 96, 54)])
def test_gpu_matches_the_model(pt, renderer_mod, scene, w, h):
    r, wl = _ctx(pt, renderer_mod, scene, w, h)
    thru = r.through_rule(**CHAINS)
    A = (wl.buffers[0], wl.buffers[1])
    B = move(*A, **SMALL)
    fr, T = _inject(w, h)
    recs_h = _records(r, thru)
    _setcam(r, *B)
    recs_n = _records(r, thru)
    k = np.ascontiguousarray(recs_n[1][..., 14]).view(np.int32)
    ys, xs = np.nonzero(k >= 1)
    on_chain = np.array([xs[len(xs) // 2], ys[len(ys) // 2], 0.0], np.float32) if len(xs) else np.array([w // 2, h // 2, 0.0], np.float32)
    for rule in RULES:
        mouse_b = on_chain if rule["tol"] == 0.02 else NO_MOUSE   # the overlay on a chain pixel (where the scene has one) in half of the cases
        _setcam(r, *A)
        r.set_buffer(2, wl.buffers[2])
        r.write_frame(fr)                                       # the image's camera: A
        r.write_moments(T)
        _setcam(r, *B)
        r.set_buffer(2, mouse_b)
        kept, kept_t = r.reproject_frame_through(thru, _rule(r, rule))
        got, gotT = r.read_frame(), r.read_moments()
        want, wantT, wkept, wkept_t, info = _want(r, wl, recs_n, recs_h, fr, T, A, B, mouse_b, rule)
        moved = int(((info["source"] >= 0) & (info["source"] != info["guess"])).sum())
        print(f"{scene} {w}x{h} {rule}: chain pixels {int(info['chain'].sum())}, kept {wkept}, kept through {wkept_t}, off the guess {moved}")
        assert frames_equal(got, want), (scene, w, h, rule, "FRAME", _differ(got, want))
        assert frames_equal(gotT, wantT), (scene, w, h, rule, "T", _differ(gotT, wantT))
        assert (kept, kept_t) == (wkept, wkept_t), (scene, w, h, rule, kept, kept_t, wkept, wkept_t)
        if (scene, w, h) in FLOORS and (rule["radius"], rule["tol"], rule["allm"]) == (2, 0.05, False):
            assert wkept_t >= FLOORS[(scene, w, h)][0] and moved >= FLOORS[(scene, w, h)][1], (wkept_t, moved)
    r.close()


@pytest.mark.parametrize("thru_kw", [dict(max_depth=0, min_weight=0.5, lobes=3, key=True), dict(max_depth=4, min_weight=0.5, lobes=0, key=False)])
def test_a_rule_without_chains_is_pt_reproject_frame(pt, renderer_mod, thru_kw):
    fr, T = _inject(W, H)
    out = []
    for through in (True, False):
        r, wl = _ctx(pt, renderer_mod, "C3")
        r.write_frame(fr)
        r.write_moments(T)
        _setcam(r, *move(wl.buffers[0], wl.buffers[1], **SMALL))
        if through:
            kept, kept_t = r.reproject_frame_through(r.through_rule(**thru_kw), r.reproject_through_rule(10.0, 0.02, 0.9, 0.05, 2))
            assert kept_t == 0
        else:
            kept = r.reproject_frame(10.0, 0.02, 0.9)
        out.append((kept, r.read_frame(), r.read_moments()))
        r.close()
    assert out[0][0] == out[1][0] and 0 < out[0][0] < W * H
    assert frames_equal(out[0][1], out[1][1]) and frames_equal(out[0][2], out[1][2])


def test_unchanged_camera_is_the_identity(pt, renderer_mod):
    """on every kept pixel, apart from the cap.  With holes in the image (no count, a NaN) that holds for the kept pixels whose own cell has a
    history; a chain pixel without one takes the nearest neighbour's on the same surface (step 5), which no first-hit pixel does"""
    r, wl = _ctx(pt, renderer_mod, "C3")
    chain = np.ascontiguousarray(r.read_features_through(r.through_rule(*r.REPROJECT_THROUGH_CHAINS))[..., 14]).view(np.int32) >= 1
    for holes in (False, True):
        fr, T = _inject(W, H)
        if not holes:
            rs = np.random.RandomState(5)
            cnt = rs.randint(1, 100, size=(H, W, 1)).astype(np.float32)
            fr = np.concatenate([rs.rand(H, W, 3).astype(np.float32) * cnt, cnt], -1)
        fr[..., :3] *= np.float32(0.5)
        fr[..., 3] = np.minimum(fr[..., 3], 50.0)               # below the cap
        T[..., 2] = np.minimum(T[..., 2], 50.0)
        r.write_frame(fr)
        r.write_moments(T)
        kept, kept_t = r.reproject_frame_through()
        got, gotT = r.read_frame(), r.read_moments()
        keep = got[..., 3] > 0
        own = (fr[..., 3] > 0) & np.isfinite(fr[..., :3]).all(-1)
        assert kept == int(keep.sum()) and kept_t == int((keep & chain).sum()) and kept_t > 300      # all but those that end on a mirror or on glass
        same = keep & own
        assert np.array_equal(got[same].view(np.uint32), fr[same].view(np.uint32)) and np.array_equal(gotT[same].view(np.uint32), T[same].view(np.uint32))
        assert not got[~keep].any() and not gotT[~keep].any()
        assert chain[keep & ~own].all() and (keep & ~own).any() == holes
    r.close()


def test_statistics_are_carried_and_capped_on_a_chain_pixel(pt, renderer_mod):
    r, wl = _ctx(pt, renderer_mod, "C3")
    thru = r.through_rule(**CHAINS)
    r.record_moments(True)
    r.render_batch(1, [pt.scenes.frame_seed(f) for f in range(1, 5)])
    _setcam(r, *move(wl.buffers[0], wl.buffers[1], **SMALL))
    chain = np.ascontiguousarray(r.read_features_through(thru)[..., 14]).view(np.int32) >= 1
    kept, kept_t = r.reproject_frame_through(thru, r.reproject_through_rule(max_history=3.0))
    F, T = r.read_frame(), r.read_moments()
    on = chain & (F[..., 3] > 0)
    assert kept_t == int(on.sum()) and kept_t > 300
    assert (F[on][:, 3] == 3).all() and (T[on][:, 2] == 3).all() and (T[on][:, 0] > 0).any()      # 4 frames capped to 3, in FRAME and on T's own n
    assert not T[chain & ~on].any()
    r.history_hold()                                            # the current inputs are the image's camera: the hold is accepted ...
    assert not r.read_frame().any()
    r.render_batch(5, [pt.scenes.frame_seed(f) for f in range(5, 7)])
    r.history_merge()                                           # ... and so is the merge
    assert (r.read_frame()[on][:, 3] >= 2).all()
    r.close()


def _sequence(pt, r, wl):
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 9)]
    r.record_moments(True)
    r.render_batch(1, seeds[:4])
    _setcam(r, *move(wl.buffers[0], wl.buffers[1], **SMALL))
    counts = r.reproject_frame_through(rule=r.reproject_through_rule(max_history=3.0))
    mid, midT = r.read_frame(), r.read_moments()
    r.render_batch(5, seeds[4:6])
    return counts, mid, midT, r.read_frame(), r.read_moments()


def test_multi_stream_context_and_later_renders(pt, renderer_mod):
    """a pt_create_multi context {0, 0} gives the one-stream result bit for bit; two more frames after the call equal the same frames on a twin
    written with the call's result through pt_write_frame + pt_write_moments"""
    r, wl = _ctx(pt, renderer_mod, "C3")
    one = _sequence(pt, r, wl)
    r.close()
    r, wl = _ctx(pt, renderer_mod, "C3", devices=[0, 0])
    two = _sequence(pt, r, wl)
    r.close()
    assert one[0] == two[0] and one[0][1] > 300 and one[0][0] > one[0][1]
    for a, b in zip(one[1:], two[1:]):
        assert frames_equal(a, b)
    r, wl = _ctx(pt, renderer_mod, "C3")
    r.record_moments(True)
    _setcam(r, *move(wl.buffers[0], wl.buffers[1], **SMALL))
    r.write_frame(one[1])
    r.write_moments(one[2])
    r.render_batch(5, [pt.scenes.frame_seed(f) for f in range(5, 7)])
    assert frames_equal(r.read_frame(), one[3]) and frames_equal(r.read_moments(), one[4])
    r.close()


def test_errors_leave_frame_and_moments_unchanged(pt, renderer_mod):
    r, wl = _ctx(pt, renderer_mod, "C3")
    fr, T = _inject(W, H)
    r.write_frame(fr)
    r.write_moments(T)
    _setcam(r, *move(wl.buffers[0], wl.buffers[1], **SMALL))
    nan = float("nan")
    good_t, good_r = dict(CHAINS), dict(max_history=64.0, depth_tol=0.02, normal_tol=0.9, point_tol=0.02, radius=2)

    def refused(code, thru=None, **kw):
        with pytest.raises(renderer_mod.PtError) as e:
            r.reproject_frame_through(r.through_rule(**{**good_t, **(thru or {})}), r.reproject_through_rule(**{**good_r, **kw}))
        assert e.value.code == code, (thru, kw, e.value.code)
        assert frames_equal(r.read_frame(), fr) and frames_equal(r.read_moments(), T), (thru, kw)

    for kw in (dict(radius=-1), dict(radius=5), dict(point_tol=0.0), dict(point_tol=-1.0), dict(point_tol=nan), dict(max_history=0.5), dict(max_history=nan),
               dict(depth_tol=0.0), dict(depth_tol=nan), dict(normal_tol=1.5), dict(normal_tol=nan)):
        refused(-1, **kw)
    for thru in (dict(key=False), dict(max_depth=9), dict(max_depth=-1), dict(min_weight=0.0), dict(min_weight=nan), dict(lobes=4)):
        refused(-1, thru=thru)
    n, nt = C.c_int64(7), C.c_int64(7)
    thru, rule = r.through_rule(**good_t), r.reproject_through_rule(**good_r)
    L = r._L.pt_reproject_frame_through
    assert L(r._h, C.byref(thru), None, C.byref(n), C.byref(nt)) == -1 and (n.value, nt.value) == (0, 0)
    assert L(r._h, None, C.byref(rule), C.byref(n), C.byref(nt)) == -1
    assert L(None, C.byref(thru), C.byref(rule), C.byref(n), C.byref(nt)) == -1
    rule.flags = 2                                              # unknown flags
    assert L(r._h, C.byref(thru), C.byref(rule), C.byref(n), C.byref(nt)) == -1
    thru.flags = 3
    assert L(r._h, C.byref(thru), C.byref(r.reproject_through_rule(**good_r)), None, None) == -1
    assert frames_equal(r.read_frame(), fr) and frames_equal(r.read_moments(), T)
    p = wl.buffers[4].copy()
    p[10] = 1.0                                                 # DEBUG
    r.set_buffer(4, p)
    refused(-5)
    p = wl.buffers[4].copy()
    p[2] = W / 2                                                # resolution no longer the image's
    r.set_buffer(4, p)
    refused(-1)
    r.set_buffer(4, wl.buffers[4])
    r.set_buffer(14, wl.buffers[14])                            # a scene upload since the camera was recorded (even the same contents)
    refused(-1)
    r.write_frame(fr)
    r.write_moments(T)
    r.set_texture(0, wl.sky)
    refused(-1)
    r.close()
    for kw in ({"shard_rank": 0, "shard_count": 2}, {"devices": [0], "first_shard": 0, "total_shards": 2}):
        r, wl = _ctx(pt, renderer_mod, "C3", **kw)
        r.render_batch(1, [pt.scenes.frame_seed(1)])
        before = r.read_frame()
        with pytest.raises(renderer_mod.PtError) as e:
            r.reproject_frame_through()
        assert e.value.code == -5, kw
        assert frames_equal(r.read_frame(), before)
        r.close()


def test_an_image_without_a_camera_is_left_alone(pt, renderer_mod):
    wl = pt.scenes.build("C3", W, H)
    r = renderer_mod.Renderer(W, H)
    fr, _ = _inject(W, H)
    r.write_frame(fr)                                           # no Parameters yet: no camera
    r.load_workload(wl)
    assert r.reproject_frame_through() == (0, 0) and frames_equal(r.read_frame(), fr)
    r.render_batch(1, [pt.scenes.frame_seed(1)])
    r.reset_frame()
    _setcam(r, *move(wl.buffers[0], wl.buffers[1], forward=0.03))
    assert r.reproject_frame_through() == (0, 0) and not r.read_frame().any()
    r.close()


def _clamped_rmse(frame, ref, where):
    img = np.where(frame[..., 3:4] > 0, frame[..., :3] / np.maximum(frame[..., 3:4], np.float32(1e-30)), 0)
    ok = where & np.isfinite(img).all(-1) & np.isfinite(ref).all(-1)
    d = np.clip(img[ok], 0, 1).astype(np.float64) - np.clip(ref[ok], 0, 1)
    return float(np.sqrt((d ** 2).mean()))


def test_carried_chain_pixels_are_less_noisy_after_a_small_move(pt, renderer_mod):
    """C3: 16 frames at A, the small move, this call and 4 frames against pt_reproject_frame (the parent: on these pixels it restarts) and the same
    4 frames; clamped RMSE over the chain pixels of B against 64 frames there"""
    r, wl = _ctx(pt, renderer_mod, "C3")
    thru = r.through_rule(**CHAINS)
    A = (wl.buffers[0], wl.buffers[1])
    B = move(*A, **SMALL)
    _setcam(r, *B)
    chain = np.ascontiguousarray(r.read_features_through(thru)[..., 14]).view(np.int32) >= 1
    r.render_batch(1, [pt.scenes.frame_seed(5000 + f) for f in range(64)])
    ref = r.read_frame()
    ref = ref[..., :3] / ref[..., 3:4]
    err = {}
    for which in ("through", "first hit"):
        _setcam(r, *A)
        r.reset_frame()
        r.render_batch(1, [pt.scenes.frame_seed(f) for f in range(1, 17)])
        _setcam(r, *B)
        kept_t = r.reproject_frame_through(thru)[1] if which == "through" else r.reproject_frame()
        r.render_batch(17, [pt.scenes.frame_seed(f) for f in range(17, 21)])
        err[which] = _clamped_rmse(r.read_frame(), ref, chain)
        if which == "through":
            assert kept_t > 300
    r.close()
    print(f"C3 {W}x{H}, {int(chain.sum())} chain pixels, clamped RMSE after 16 + 4 frames: through {err['through']:.4f}, pt_reproject_frame {err['first hit']:.4f}")
    assert err["through"] < err["first hit"], err
