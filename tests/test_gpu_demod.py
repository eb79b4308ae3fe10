"""GPU: albedo demodulation for the guided filter, its selection and the reprojection (include/pt_demod.h) against the float32 model of
tests/_demod_model.py, on the feature records of real scenes: the filter to the filter's tolerance, the selection with tests/test_gpu_steer.py's
rule, the reprojection bit for bit."""
import ctypes as C

import numpy as np
import pytest

from _demod_model import denoise_guided_demod as model
from _demod_model import reproject_demod, select_guided_demod
from _denoise_model import classify
from _reproject_model import cam_rot, frame_in, material_flags, overlay
from conftest import frames_equal
from test_gpu_guided import _inject
from test_gpu_reproject import _inject as _inject_frame
from test_gpu_reproject import move
from test_gpu_steer import _check_select

pytestmark = pytest.mark.gpu

W, H = 96, 54
INF = float("inf")
FLOOR = 0.01
HIGH_FLOOR = 0.85                                       # above some Kd channel of every scene here
# (iterations, sigmas, min_frames, albedo_floor)
CASES = [(5, (2.0, 0.3, 0.05, INF), 4, FLOOR), (3, (1.0, INF, 0.1, 0.1), 2, 0.05), (0, (2.0, 0.3, 0.05, 0.1), 4, FLOOR),
         (2, (INF, 0.3, 0.05, 0.1), 4, HIGH_FLOOR), (8, (10.0, 0.2, 0.02, INF), 6, 1e-3)]


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _seeds(pt, first, n):
    return [pt.scenes.frame_seed(f) for f in range(first, first + n)]


def _open(pt, renderer_mod, scene, w=W, h=H, **kw):
    wl = pt.scenes.build(scene, w, h)
    r = renderer_mod.Renderer(w, h, **kw)
    r.load_workload(wl)
    return r, wl


def _setcam(r, origin, rotation):
    r.set_buffer(0, np.asarray(origin, np.float32))
    r.set_buffer(1, np.asarray(rotation, np.float32))


def _map_kd_pixels(wl, feat):
    """the valid hits whose material has a map_Kd (slot 23 of its MATERIALS record)"""
    mtl = np.asarray(wl.buffers[14], np.float32)
    me = int(mtl[0])
    textured = np.array([int(mtl[me * m + 23]) >= 0 for m in range((mtl.size - 1) // me)], bool)
    mat = np.ascontiguousarray(feat[..., 11]).view(np.int32)
    hit = np.ascontiguousarray(feat[..., 7]).view(np.int32) >= 0
    ok = hit & (mat >= 0) & (mat < textured.size)
    out = np.zeros(mat.shape, bool)
    out[ok] = textured[mat[ok]]
    return out


# ---------------------------------------------------------------------------------------------------------------- filter

@pytest.mark.parametrize("scene", ["T1", "C3", "C6"])
def test_filter_matches_the_model(pt, renderer_mod, scene):
    r, _ = _open(pt, renderer_mod, scene)
    feat = r.read_features()
    fr, T = _inject(feat)
    r.write_frame(fr)
    r.write_moments(T)
    hit = classify(fr, feat)[1] == 1
    assert (feat[..., 4:7][hit] < HIGH_FLOOR).any() and (feat[..., 4:7][hit] > FLOOR).all(-1).any()
    for it, sig, mf, floor in CASES:
        got = r.denoise_guided(it, *sig, min_frames=mf, albedo_floor=floor)
        want = model(fr, feat, T, it, *sig, mf, floor)
        assert np.allclose(got, want, rtol=1e-4, atol=1e-6, equal_nan=True), (scene, it, sig, mf, floor, np.nanmax(np.abs(got - want)))
        assert np.array_equal(got[..., 3], fr[..., 3])
    assert _bits_equal(r.read_frame(), fr) and _bits_equal(r.read_moments(), T)     # neither is modified
    r.close()


def test_zero_iterations_are_within_two_ulp_of_the_mean(pt, renderer_mod):
    r, _ = _open(pt, renderer_mod, "T1")
    r.record_moments(True)
    r.render_batch(1, _seeds(pt, 1, 3))
    fr = r.read_frame()
    got = r.denoise_guided(0, albedo_floor=FLOOR)
    r.close()
    mean = fr[..., :3] / fr[..., 3:4]
    ok = np.isfinite(mean).all(-1)
    ulp = np.spacing(np.abs(mean[ok]))
    assert (np.abs(got[..., :3][ok].astype(np.float64) - mean[ok]) <= 2.0 * ulp).all()


def test_a_checker_albedo_over_constant_illumination_comes_back(pt, renderer_mod):
    """FRAME = a_p * E * n over T1's own features: the illumination is the constant E up to one rounding, so with the luminance and albedo terms
    off the demodulated filter returns the input.  Bound: a pass is sum(w c) / sum(w) over at most 25 taps whose c lie within 1 ulp of E, at most
    27 roundings of 2^-24 each = 1.6e-6 per pass, 8e-6 for the 5 passes, plus the division and the multiplication by a: below 1e-5.  The plain
    filter, told the same, blurs the checker."""
    w, h, n, E = 192, 108, 8.0, np.float32(0.6)
    r, wl = _open(pt, renderer_mod, "T1", w, h)
    feat = r.read_features()
    fr = np.zeros((h, w, 4), np.float32)
    fr[..., 3] = n
    _, cls = classify(fr, feat)                         # a zero image is finite: the classes are the features'
    a = np.where((cls == 1)[..., None], np.maximum(feat[..., 4:7], np.float32(FLOOR)), np.float32(1)).astype(np.float32)
    c = np.where((cls == 1)[..., None], a * E, np.float32(0.25)).astype(np.float32)
    fr[..., :3] = c * np.float32(n)
    Y = (np.float32(0.2126) * c[..., 0] + np.float32(0.7152) * c[..., 1]) + np.float32(0.0722) * c[..., 2]
    T = np.stack([Y * n, Y * Y * n * np.float32(1.2), np.full((h, w), n, np.float32), np.zeros((h, w), np.float32)], -1).astype(np.float32)
    r.write_frame(fr)
    r.write_moments(T)
    got = r.denoise_guided(5, INF, sigma_albedo=INF, albedo_floor=FLOOR)
    plain = r.denoise_guided(5, INF, sigma_albedo=INF)
    r.close()
    valid = cls != 0
    tex = _map_kd_pixels(wl, feat) & (cls == 1)
    assert tex.sum() > 0.05 * w * h and len(np.unique(feat[..., 4][tex])) >= 2         # the floor, with both texels of the checker
    rel = np.abs(got[..., :3][valid] / c[valid] - 1)
    assert rel.max() <= 1e-5, float(rel.max())
    assert np.abs(plain[..., :3][tex] / c[tex] - 1).max() > 0.01


@pytest.mark.parametrize("java_bytes", [True, False])
def test_display_is_the_display_conversion(pt, oracle, renderer_mod, java_bytes):
    r, _ = _open(pt, renderer_mod, "T1")
    r.record_moments(True)
    r.render_batch(1, _seeds(pt, 1, 3))
    dn = r.denoise_guided(4, sigma_albedo=INF, albedo_floor=FLOOR)
    disp = r.read_display_denoised_guided(4, sigma_albedo=INF, java_bytes=java_bytes, albedo_floor=FLOOR)
    plain = r.denoise_guided(4, sigma_albedo=INF)
    r.close()
    assert np.array_equal(disp, oracle.display(dn, 1, java_bytes))
    assert not np.array_equal(dn, plain)                # the demodulated call is another filter


def test_multi_stream_equals_single(pt, renderer_mod):
    out = []
    for kw in ({}, {"devices": [0, 0]}):
        r, _ = _open(pt, renderer_mod, "T1", **kw)
        r.record_moments(True)
        r.render_batch(1, _seeds(pt, 1, 3))
        out.append((r.read_frame(), r.read_moments(), r.denoise_guided(5, albedo_floor=FLOOR), r.select_guided(0.05, albedo_floor=FLOOR)))
        r.close()
    for a, b in zip(*out):
        assert _bits_equal(a, b) if a.dtype == np.float32 else np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- selection

SMOUSE = np.array([30.0, 17.0, 0.0], np.float32)
# (iterations, sigmas, min_frames, rel_err, abs_err, max_frames, albedo_floor).  The band in which the device may decide either way is the step-5
# pixels within 1e-3 relative of the threshold.  The model's own share of such pixels, on the injected image over the feature records of T1, C3
# and C6 at this size: at most 0.08 % of the pixels for any rule and scene (4 of 5184), 0.02 % over all of them; the test's condition is 1 %.
RULES = [(5, (2.0, 0.3, 0.05, INF), 4, 0.05, 0.0, 0, FLOOR), (0, (2.0, 0.3, 0.05, 0.1), 4, 0.1, 0.0, 0, 0.05), (3, (1.0, INF, 0.1, INF), 2, 0.02, 0.001, 7, FLOOR),
         (2, (INF, 0.3, 0.05, 0.1), 4, 0.3, 0.0, 0, HIGH_FLOOR), (8, (10.0, 0.2, 0.02, 0.05), 6, 0.01, 0.0, 5, 1e-3)]


def _select_raw(r, rule, floor):
    out = np.zeros((r.H, r.W), np.uint8)
    n = C.c_int64(-1)
    assert r._L.pt_select_guided_demod(r._h, C.byref(rule), floor, out.ctypes.data, C.byref(n)) == 0
    assert set(np.unique(out)) <= {0, 1}
    return out.astype(bool), n.value


@pytest.mark.parametrize("scene", ["T1", "C3", "C6"])
def test_select_matches_the_model(pt, renderer_mod, scene):
    r, wl = _open(pt, renderer_mod, scene)
    r.set_buffer(2, SMOUSE)
    ov = overlay(W, H, frame_in(wl.buffers[4], wl.buffers[0], wl.buffers[1], SMOUSE))
    assert ov.any()
    feat = r.read_features()
    fr, T = _inject(feat)
    T2 = T.copy()                                       # n >= 8 and no NaN sum: step 5 compares finite variances everywhere (tests/test_gpu_steer.py)
    T2[..., 2] = np.maximum(T2[..., 2], 8.0)
    T2[40, 50, :2] = (4.0, 3.0)
    steps = set()
    for moments, rules in ((T, RULES), (T2, [rule[:5] + (0,) + rule[6:] for rule in RULES])):
        r.write_frame(fr)
        r.write_moments(moments)
        for it, sig, mf, rel, ab, mx, floor in rules:
            got, n = _select_raw(r, r.guided_rule(rel, ab, it, *sig, min_frames=mf, max_frames=mx), floor)
            want, d = select_guided_demod(fr, feat, moments, it, *sig, mf, rel, ab, mx, floor=floor, overlay=ov, detail=True)
            _check_select(got, n, want, d)
            assert np.array_equal(r.select_guided(rel, ab, it, *sig, min_frames=mf, max_frames=mx, albedo_floor=floor), got)
            steps |= set(np.unique(d["step"]).tolist())
        assert _bits_equal(r.read_frame(), fr) and _bits_equal(r.read_moments(), moments)      # neither is modified
    assert steps == {1, 2, 3, 4, 5}                                     # every step decided some pixel
    r.close()


# (first, n, rel_err, min_frames, max_frames) of successive calls
GCALLS = [(1, 2, 0.05, 2, 0), (3, 2, 0.05, 2, 0), (5, 2, 0.05, 4, 0), (7, 2, 0.02, 4, 9), (9, 2, 0.05, 4, 0)]


def _guided_run(pt, renderer_mod, split, **kw):
    r, _ = _open(pt, renderer_mod, "T1", 128, 72, **kw)
    r.reset_frame()
    counts = []
    for first, n, rel, mf, mx in GCALLS:
        if split:
            mask = r.select_guided(rel, min_frames=mf, max_frames=mx, sigma_albedo=INF, albedo_floor=FLOOR)
            counts.append(r.render_mask(first, _seeds(pt, first, n), mask))
        else:
            counts.append(r.render_adaptive_guided(first, _seeds(pt, first, n), rel, min_frames=mf, max_frames=mx, sigma_albedo=INF, albedo_floor=FLOOR))
    out = (counts, r.read_frame(), r.read_moments())
    r.close()
    return out


def test_render_adaptive_guided_demod_is_select_then_mask(pt, renderer_mod):
    runs = {(split, multi): _guided_run(pt, renderer_mod, split, **({"devices": [0, 0]} if multi else {}))
            for split in (False, True) for multi in (False, True)}
    base = runs[(False, False)]
    assert base[0][0] == 128 * 72                                        # no moments yet: every pixel
    assert any(0 < c < base[0][0] for c in base[0][1:]), base[0]         # a real selection afterwards
    for key, (counts, F, T) in runs.items():
        assert counts == base[0], key
        assert frames_equal(F, base[1]) and _bits_equal(T, base[2]), key


# ---------------------------------------------------------------------------------------------------------------- reprojection

def _want(r, wl, rn, rh, fr, T, A, B, mouse_b, mh=64.0, dt=0.02, nt=0.9, allm=False, floor=FLOOR):
    cos = lambda x: r.debug_math("cos", x)      # noqa: E731  (the shader's own functions, as k_frame_setup calls them)
    sin = lambda x: r.debug_math("sin", x)      # noqa: E731
    fin_a = frame_in(wl.buffers[4], A[0], A[1], wl.buffers[2])
    fin_b = frame_in(wl.buffers[4], B[0], B[1], mouse_b)
    return reproject_demod(rn, rh, fr, T, fin_a, fin_b, material_flags(wl.buffers[14]), cam_rot(A[1], cos, sin), mh, dt, nt, allm, floor)


def _inject_moments(fr, seed=9):
    rs = np.random.RandomState(seed)
    h, w = fr.shape[:2]
    n = rs.randint(0, 100, size=(h, w)).astype(np.float32)
    Y = rs.rand(h, w).astype(np.float32)
    return np.stack([n * Y, n * Y * Y * (1.0 + rs.rand(h, w) * 0.5), n, np.zeros_like(n)], -1).astype(np.float32)


RCASES = [dict(mh=64.0, dt=0.02, nt=0.9, allm=False, floor=FLOOR), dict(mh=10.0, dt=0.05, nt=0.5, allm=True, floor=HIGH_FLOOR)]


@pytest.mark.parametrize("scene", ["T1", "C2"])
def test_reprojection_matches_the_model_bit_for_bit(pt, renderer_mod, scene):
    r, wl = _open(pt, renderer_mod, scene)
    A = (wl.buffers[0], wl.buffers[1])
    rh = r.read_features()
    fr = _inject_frame()
    T = _inject_moments(fr)
    changed = 0
    for step, (fwd, strafe, yaw) in enumerate([(0.03, 0.02, 0.02), (-0.05, 0.0, -0.03)]):
        B = move(*A, forward=fwd, strafe=strafe, yaw=yaw)
        mouse_b = np.array([30.0, 17.0, 0.0] if step else [-1.0e6, -1.0e6, 0.0], np.float32)
        for case in RCASES:
            _setcam(r, *A)
            r.set_buffer(2, wl.buffers[2])
            r.write_frame(fr)                                   # the image's camera: A
            r.write_moments(T)
            _setcam(r, *B)
            r.set_buffer(2, mouse_b)
            rn = r.read_features()
            kept = r.reproject_frame(case["mh"], case["dt"], case["nt"], case["allm"], albedo_floor=case["floor"])
            got, gotT = r.read_frame(), r.read_moments()
            want, wantT, wkept = _want(r, wl, rn, rh, fr, T, A, B, mouse_b, **case)
            assert frames_equal(got, want), (scene, step, case, int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum()))
            assert frames_equal(gotT, wantT), (scene, step, case, int((gotT.view(np.uint32) != wantT.view(np.uint32)).any(-1).sum()))
            assert kept == wkept and 0 < kept < W * H, (scene, step, case, kept, wkept)
            # against the plain call: the same pixels kept, and (T1's textured floor) other sums where the texel changed
            _setcam(r, *A)
            r.set_buffer(2, wl.buffers[2])
            r.write_frame(fr)
            _setcam(r, *B)
            r.set_buffer(2, mouse_b)
            assert r.reproject_frame(case["mh"], case["dt"], case["nt"], case["allm"]) == kept
            plain = r.read_frame()
            assert np.array_equal(plain[..., 3], got[..., 3])
            changed += int((plain[..., :3] != got[..., :3]).any(-1).sum())
    if scene == "T1":
        assert changed > 0                                      # the texture moved under some kept pixel
    r.close()


def test_reprojection_with_an_unchanged_camera_is_the_identity(pt, renderer_mod):
    for scene in ("T1", "C2"):
        r, wl = _open(pt, renderer_mod, scene)
        fr = _inject_frame()
        fr[..., :3] *= np.float32(0.5)
        fr[..., 3] = np.minimum(fr[..., 3], 50.0)              # below the cap
        T = _inject_moments(fr)
        T[..., 2] = np.minimum(T[..., 2], 50.0)
        r.write_frame(fr)
        r.write_moments(T)
        kept = r.reproject_frame(albedo_floor=FLOOR)
        got, gotT = r.read_frame(), r.read_moments()
        keep = got[..., 3] > 0
        assert kept == int(keep.sum()) and kept > 0
        assert np.array_equal(got[keep].view(np.uint32), fr[keep].view(np.uint32))
        assert np.array_equal(gotT[keep].view(np.uint32), T[keep].view(np.uint32))
        assert not got[~keep].any() and not gotT[~keep].any()
        r.write_frame(fr)
        assert r.reproject_frame() == kept and frames_equal(r.read_frame(), got)       # the plain call keeps the same pixels
        r.close()


def _sequence(pt, r, wl):
    A = (wl.buffers[0], wl.buffers[1])
    r.render_adaptive(1, _seeds(pt, 1, 4), 0.0, 0.0, min_frames=100)
    _setcam(r, *move(*A, forward=0.04, strafe=0.03, yaw=0.03))
    kept = r.reproject_frame(max_history=3.0, albedo_floor=FLOOR)
    mid, midT = r.read_frame(), r.read_moments()
    n = r.render_adaptive(5, _seeds(pt, 5, 2), 0.0, 1e30, min_frames=3)
    return kept, mid, midT, n, r.read_frame()


def test_multi_stream_context_reprojects_as_one_stream(pt, renderer_mod):
    out = []
    for kw in ({}, {"devices": [0, 0]}):
        r, wl = _open(pt, renderer_mod, "T1", **kw)
        out.append(_sequence(pt, r, wl))
        r.close()
    (k0, m0, t0, n0, f0), (k1, m1, t1, n1, f1) = out
    assert 0 < k0 < W * H and n0 == W * H - k0
    assert k0 == k1 and n0 == n1
    assert frames_equal(m0, m1) and frames_equal(t0, t1) and frames_equal(f0, f1)


def test_renders_after_a_reprojection_equal_renders_on_its_written_image(pt, renderer_mod):
    r, wl = _open(pt, renderer_mod, "T1")
    A = (wl.buffers[0], wl.buffers[1])
    B = move(*A, forward=0.02, strafe=-0.02, yaw=-0.02)
    r.render_batch(1, _seeds(pt, 1, 4))
    _setcam(r, *B)
    r.reproject_frame(albedo_floor=FLOOR)
    mid = r.read_frame()
    r.render_batch(5, _seeds(pt, 5, 5))
    got = r.read_frame()
    r.close()
    r2, _ = _open(pt, renderer_mod, "T1")
    _setcam(r2, *B)
    r2.write_frame(mid)
    r2.render_batch(5, _seeds(pt, 5, 5))
    want = r2.read_frame()
    r2.close()
    assert frames_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- errors

def test_errors_and_unsupported_contexts(pt, renderer_mod):
    PtError = renderer_mod.PtError
    r, wl = _open(pt, renderer_mod, "T1")
    r.record_moments(True)
    r.render_batch(1, _seeds(pt, 1, 3))
    _setcam(r, *move(wl.buffers[0], wl.buffers[1], forward=0.03))
    F, T = r.read_frame(), r.read_moments()
    seeds = _seeds(pt, 4, 2)
    for floor in (0.0, -0.01, float("nan"), INF):
        for call in (lambda: r.denoise_guided(albedo_floor=floor), lambda: r.read_display_denoised_guided(albedo_floor=floor),
                     lambda: r.select_guided(0.05, albedo_floor=floor), lambda: r.render_adaptive_guided(4, seeds, 0.05, albedo_floor=floor),
                     lambda: r.reproject_frame(albedo_floor=floor)):
            with pytest.raises(PtError) as e:
                call()
            assert e.value.code == -1, floor                    # PT_ERR_ARG
    # the plain calls' own checks still hold
    for call in (lambda: r.denoise_guided(9, albedo_floor=FLOOR), lambda: r.denoise_guided(2, 0.0, albedo_floor=FLOOR),
                 lambda: r.denoise_guided(2, min_frames=1, albedo_floor=FLOOR), lambda: r.select_guided(-0.1, albedo_floor=FLOOR),
                 lambda: r.render_adaptive_guided(4, seeds, 0.05, iterations=9, albedo_floor=FLOOR),
                 lambda: r.reproject_frame(0.5, albedo_floor=FLOOR), lambda: r.reproject_frame(64, 0.0, albedo_floor=FLOOR)):
        with pytest.raises(PtError) as e:
            call()
        assert e.value.code == -1
    L, h = r._L, r._h
    n = C.c_int64(7)
    out = np.zeros((H, W, 4), np.float32)
    mask = np.zeros((H, W), np.uint8)
    good = r.guided_rule(0.05)
    sd = np.array(seeds, np.int32).ctypes.data
    assert L.pt_reproject_frame_demod(h, 64.0, 0.02, 0.9, 2, FLOOR, C.byref(n)) == -1 and n.value == 0          # unknown flags
    assert L.pt_reproject_frame_demod(None, 64.0, 0.02, 0.9, 0, FLOOR, C.byref(n)) == -1
    assert L.pt_denoise_guided_demod(h, 1, 2.0, 0.3, 0.05, 0.1, 4, FLOOR, None) == -1
    assert L.pt_denoise_guided_demod(None, 1, 2.0, 0.3, 0.05, 0.1, 4, FLOOR, out.ctypes.data) == -1
    assert L.pt_read_display_denoised_guided_demod(h, 1, 2.0, 0.3, 0.05, 0.1, 4, FLOOR, 1, None) == -1
    assert L.pt_select_guided_demod(None, C.byref(good), FLOOR, mask.ctypes.data, None) == -1
    assert L.pt_select_guided_demod(h, None, FLOOR, mask.ctypes.data, None) == -1
    assert L.pt_select_guided_demod(h, C.byref(good), FLOOR, None, C.byref(n)) == -1 and n.value == 0
    assert L.pt_render_adaptive_guided_demod(None, 4, 2, sd, C.byref(good), FLOOR, None) == -1
    assert L.pt_render_adaptive_guided_demod(h, 4, 2, None, C.byref(good), FLOOR, None) == -1
    assert L.pt_render_adaptive_guided_demod(h, 4, 2, sd, None, FLOOR, None) == -1
    assert L.pt_render_adaptive_guided_demod(h, 4, 0, sd, C.byref(good), FLOOR, C.byref(n)) == -1 and n.value == 0
    assert frames_equal(r.read_frame(), F) and _bits_equal(r.read_moments(), T)      # no failed call touched FRAME or T
    r.close()
    r, _ = _open(pt, renderer_mod, "T1")                # no moments: the filter refuses, as the plain one
    r.render_batch(1, _seeds(pt, 1, 2))
    with pytest.raises(PtError) as e:
        r.denoise_guided(albedo_floor=FLOOR)
    assert e.value.code == -1 and "pt_record_moments" in str(e.value)
    r.close()
    for kw in (dict(shard_rank=0, shard_count=2), dict(devices=[0], first_shard=0, total_shards=2)):
        p, _ = _open(pt, renderer_mod, "T1", **kw)
        p.record_moments(True)
        p.render_batch(1, _seeds(pt, 1, 2))
        Fp = p.read_frame()
        for call in (lambda: p.denoise_guided(albedo_floor=FLOOR), lambda: p.read_display_denoised_guided(albedo_floor=FLOOR),
                     lambda: p.select_guided(0.05, albedo_floor=FLOOR), lambda: p.render_adaptive_guided(3, seeds, 0.05, albedo_floor=FLOOR),
                     lambda: p.reproject_frame(albedo_floor=FLOOR)):
            with pytest.raises(PtError) as e:
                call()
            assert e.value.code == -5, kw                       # PT_ERR_UNSUPPORTED
        assert frames_equal(p.read_frame(), Fp)
        p.close()


# ---------------------------------------------------------------------------------------------------------------- sizes

MARGIN = 24     # how far a filtered pixel sees: 3 passes reach 2 * (1 + 2 + 4) = 14 pixels, the pooled variance 3 more


def _windows(w, h, wh=72, ww=112):
    """(y0, y1, x0, x1, inner) of model windows: the whole image when it is small, else the four corners, the centre and two more; inner = the
    window's pixels at least MARGIN away from every window edge that is not an image edge (there the window's model is the image's)"""
    if h <= wh or w <= ww:
        yield 0, h, 0, w, np.ones((h, w), bool)
        return
    for y0, x0 in ((0, 0), (0, w - ww), (h - wh, 0), (h - wh, w - ww), ((h - wh) // 2, (w - ww) // 2), (h // 3, 64 * 7 - 40), (h - wh - 3, w // 5)):
        y1, x1 = y0 + wh, x0 + ww
        yy, xx = np.mgrid[y0:y1, x0:x1]
        inner = ((yy - y0 >= MARGIN) | (y0 == 0)) & ((y1 - 1 - yy >= MARGIN) | (y1 == h)) & ((xx - x0 >= MARGIN) | (x0 == 0)) & \
                ((x1 - 1 - xx >= MARGIN) | (x1 == w))
        yield y0, y1, x0, x1, inner


@pytest.mark.parametrize("w,h", [(1920, 1080), (100, 7)])           # 100 x 7: a partial block of 64 columns, every block below its row count
def test_full_size_and_edge_shapes(pt, renderer_mod, w, h):
    """T1 at w x h: 4 recorded frames, then the demodulated filter and selection against the model on windows of the image (the model of a whole
    1080p image takes minutes), a move, and the demodulated reprojection of FRAME and T against its model over the whole image, bit for bit"""
    r, wl = _open(pt, renderer_mod, "T1", w, h)
    r.record_moments(True)
    r.render_batch(1, _seeds(pt, 1, 4))
    fr, T, feat = r.read_frame(), r.read_moments(), r.read_features()
    it, sig, mf, floor, rel = 3, (2.0, 0.3, 0.05, INF), 6, FLOOR, 0.05       # min_frames 6 > n = 4: every variance is pooled
    got = r.denoise_guided(it, *sig, min_frames=mf, albedo_floor=floor)
    rule = r.guided_rule(rel, 0.0, it, *sig, min_frames=4)
    sel, n_sel = _select_raw(r, rule, floor)
    assert n_sel == int(sel.sum()) and 0 < n_sel < w * h
    assert np.array_equal(got[..., 3], fr[..., 3])
    compared = 0
    for y0, y1, x0, x1, inner in _windows(w, h):
        sub = (slice(y0, y1), slice(x0, x1))
        want = model(fr[sub], feat[sub], T[sub], it, *sig, mf, floor)
        assert np.allclose(got[sub][inner], want[inner], rtol=1e-4, atol=1e-6, equal_nan=True), (w, h, y0, x0, np.nanmax(np.abs(got[sub][inner] - want[inner])))
        wsel, d = select_guided_demod(fr[sub], feat[sub], T[sub], it, *sig, 4, rel, 0.0, 0, floor=floor, detail=True)
        _check_select(sel[sub][inner], int(sel[sub][inner].sum()), wsel[inner], {k: v[inner] for k, v in d.items()})
        compared += int(inner.sum())
    assert compared >= min(w * h, 7 * 24 * 64)
    assert _bits_equal(r.read_frame(), fr) and _bits_equal(r.read_moments(), T)
    A = (wl.buffers[0], wl.buffers[1])
    B = move(*A, forward=0.02, strafe=0.01, yaw=0.01)
    _setcam(r, *B)
    rn = r.read_features()
    case = dict(mh=3.0, dt=0.02, nt=0.9, allm=True, floor=floor)       # max_history 3 < 4 frames: every kept pixel is capped
    kept = r.reproject_frame(case["mh"], case["dt"], case["nt"], case["allm"], albedo_floor=floor)
    gotF, gotT = r.read_frame(), r.read_moments()
    want, wantT, wkept = _want(r, wl, rn, feat, fr, T, A, B, wl.buffers[2], **case)
    r.close()
    assert frames_equal(gotF, want), (w, h, int((gotF.view(np.uint32) != want.view(np.uint32)).any(-1).sum()))
    assert frames_equal(gotT, wantT), (w, h, int((gotT.view(np.uint32) != wantT.view(np.uint32)).any(-1).sum()))
    assert kept == wkept and 0 < kept < w * h
