"""GPU: interleaved rendering (include/pt_fill.h).  pt_render_interleaved bit for bit against pt_render_mask with the lattice's mask and against
the oracle's strided frames; pt_fill_frame and pt_denoise_guided_filled against the float32 model of tests/_fill_model.py on the feature records
of real scenes, to the filters' tolerance, the filled count exactly."""
import ctypes as C

import numpy as np
import pytest

from _fill_model import denoise_guided_filled as model
from _fill_model import fill_frame, lattice
from conftest import frames_equal
from test_gpu_demod import _windows
from test_gpu_guided import _inject

pytestmark = pytest.mark.gpu

W, H = 96, 54
INF = float("inf")
# The fill's (sigma_normal, sigma_depth, sigma_albedo).  A tap weight is h h exp(-e) with h h >= 1/256.  SAFE keeps every weight away from the 1e-30
# cut by construction: |N_p - N_q|^2 <= 4 and |Kd_p - Kd_q|^2 <= 3 give e <= 4 / 0.35^2 + 3 / 0.35^2 = 57.2, w >= 5e-28.  REAL is the renderer's
# default; that no weight of a case lies within a factor 100 of the cut is asserted from the model (_check_fill).
REAL, SAFE, OFF = (0.3, 0.05, INF), (0.35, INF, 0.35), (INF, INF, INF)
FLOORS = (0.0, 0.2)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _seeds(pt, first, n):
    return [pt.scenes.frame_seed(f) for f in range(first, first + n)]


def _open(pt, renderer_mod, scene, w=W, h=H, **kw):
    wl = pt.scenes.build(scene, w, h)
    r = renderer_mod.Renderer(w, h, **kw)
    r.load_workload(wl)
    r.reset_frame()
    return r, wl


# ---------------------------------------------------------------------------------------------------------------- pt_render_interleaved

# (w, h, stride, phase_x, phase_y, context)
LATTICES = [(W, H, 2, 0, 0, {}), (W, H, 2, 1, 0, {}), (W, H, 2, 0, 1, {}), (W, H, 2, 1, 1, {}), (W, H, 3, 2, 1, {}), (W, H, 1, 0, 0, {}),
            (100, 37, 3, 1, 2, {}), (100, 37, 8, 7, 5, {}), (W, H, 2, 1, 0, {"devices": [0, 0]})]


@pytest.mark.parametrize("w,h,stride,px,py,ctx", LATTICES)
def test_render_interleaved_is_render_mask_on_the_lattice(pt, oracle, renderer_mod, w, h, stride, px, py, ctx):
    mask = lattice(h, w, stride, px, py)
    assert mask.any() and (stride == 1) == bool(mask.all())
    calls = [(1, 2), (3, 1)]                             # frame 1 first (it overwrites FRAME), then one more on the same lattice
    out = []
    for interleaved in (True, False):
        r, wl = _open(pt, renderer_mod, "C3", w, h, **ctx)
        counts = []
        for first, n in calls:
            if interleaved:
                counts.append(r.render_interleaved(first, _seeds(pt, first, n), stride, px, py))
            else:
                counts.append(r.render_mask(first, _seeds(pt, first, n), mask))
        out.append((counts, r.read_frame(), r.read_moments()))
        r.close()
    (c0, F0, T0), (c1, F1, T1) = out
    assert c0 == c1 == [int(mask.sum())] * 2
    assert frames_equal(F0, F1) and _bits_equal(T0, T1)
    want, _ = oracle.render_frames(oracle.Scene.from_workload(wl), w, h, 1, 3, _seeds(pt, 1, 3), nthreads=8, x0=px, xs=stride, y0=py, ys=stride)
    assert frames_equal(F0, want) and frames_equal(F1, want)
    assert (F0[..., 3][mask] == 3).all() and not F0[~mask].any() and np.array_equal(T0[..., 2], F0[..., 3])


def test_interleaved_phases_complete_the_image(pt, oracle, renderer_mod):
    """the four phases of stride 2, one call each with the same frame: together the full frame, bit for bit"""
    r, wl = _open(pt, renderer_mod, "C3")
    total = sum(r.render_interleaved(1, _seeds(pt, 1, 1), 2, px, py) for py in (0, 1) for px in (0, 1))
    got = r.read_frame()
    r.close()
    want, _ = oracle.render_frames(oracle.Scene.from_workload(wl), W, H, 1, 1, _seeds(pt, 1, 1), nthreads=8)
    assert total == W * H and frames_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- the fill and the filter

def _holes(fr, T):
    """the injected image of tests/test_gpu_guided.py with holes: everything off the (1, 0) lattice of stride 2 in the left two thirds, a block
    of nothing but holes (its inside finds no source), scattered holes in the fully rendered rest, some with raw rgb under a zero or negative
    count"""
    fr, T = fr.copy(), T.copy()
    h, w = fr.shape[:2]
    hole = ~lattice(h, w, 2, 1, 0)
    hole[:, 2 * w // 3:] = np.random.RandomState(3).rand(h, w - 2 * w // 3) < 0.2
    hole[30:42, 8:20] = True
    fr[hole] = 0.0
    T[hole] = 0.0
    fr[5, 6] = (0.5, 0.25, 0.125, 0.0)
    fr[7, 70] = (1.0, 2.0, 3.0, -2.0)
    return fr, T, hole


def _check_fill(r, fr, feat, geo, floor):
    got, n = r.fill_frame(*geo, albedo_floor=floor if floor else None)
    want, wn, d = fill_frame(fr, feat, *geo, floor, detail=True)
    assert d["margin"].min() >= 100.0, (geo, floor, float(d["margin"].min()))      # no weight near the cut: the count cannot pass by luck
    assert n == wn, (geo, floor, n, wn)
    assert np.array_equal(got[..., 3] > 0, want[..., 3] > 0)
    assert np.allclose(got, want, rtol=1e-4, atol=1e-6, equal_nan=True), (geo, floor, np.nanmax(np.abs(got - want)))
    keep = ~d["filled"]
    assert _bits_equal(got[keep], fr[keep])             # every pixel that was not filled, bit for bit
    return d


@pytest.mark.parametrize("scene", ["C3", "T1"])
def test_fill_and_filter_match_the_model(pt, renderer_mod, scene):
    r, _ = _open(pt, renderer_mod, scene)
    feat = r.read_features()
    fr, T, hole = _holes(*_inject(feat))
    r.write_frame(fr)
    r.write_moments(T)
    for geo in (REAL, SAFE, OFF):
        for floor in FLOORS:
            d = _check_fill(r, fr, feat, geo, floor)
            assert 0.5 * hole.sum() < d["filled"].sum() < d["hole"].sum() <= (fr[..., 3] <= 0).sum()      # some holes find nothing
    for it, lum_sigma, geo, mf in ((5, 2.0, REAL, 4), (3, 1.0, SAFE, 2), (0, 2.0, REAL, 4), (2, INF, OFF, 6)):
        for floor in FLOORS:
            got = r.denoise_guided(it, lum_sigma, *geo, min_frames=mf, albedo_floor=floor if floor else None, fill=True)
            want = model(fr, feat, T, it, lum_sigma, *geo, mf, floor)
            assert np.allclose(got, want, rtol=1e-4, atol=1e-6, equal_nan=True), (scene, it, geo, mf, floor, np.nanmax(np.abs(got - want)))
            assert np.array_equal(got[..., 3], fr[..., 3])          # the real count: 0 marks a reconstructed pixel
    assert _bits_equal(r.read_frame(), fr) and _bits_equal(r.read_moments(), T)     # neither is modified
    r.close()


def test_an_image_without_holes_gives_the_plain_calls_bit_for_bit(pt, renderer_mod):
    r, _ = _open(pt, renderer_mod, "T1")
    r.record_moments(True)
    r.render_batch(1, _seeds(pt, 1, 3))
    fr, T = r.read_frame(), r.read_moments()
    assert (fr[..., 3] > 0).all()
    for floor in FLOORS:
        got, n = r.fill_frame(albedo_floor=floor if floor else None)
        assert n == 0 and _bits_equal(got, fr)
    for it in (0, 4):
        assert _bits_equal(r.denoise_guided(it, fill=True), r.denoise_guided(it))
        assert _bits_equal(r.denoise_guided(it, sigma_albedo=INF, albedo_floor=0.2, fill=True), r.denoise_guided(it, sigma_albedo=INF, albedo_floor=0.2))
    assert np.array_equal(r.read_display_denoised_guided(4, fill=True), r.read_display_denoised_guided(4))
    assert _bits_equal(r.read_frame(), fr) and _bits_equal(r.read_moments(), T)
    r.close()


def test_an_image_of_nothing_but_holes_is_left_alone(pt, renderer_mod):
    r, _ = _open(pt, renderer_mod, "C3")
    r.record_moments(True)                              # T allocated, and zero
    zero = np.zeros((H, W, 4), np.float32)
    for floor in FLOORS:
        got, n = r.fill_frame(albedo_floor=floor if floor else None)
        assert n == 0 and _bits_equal(got, zero)
        assert _bits_equal(r.denoise_guided(5, albedo_floor=floor if floor else None, fill=True), zero)
    assert not r.read_display_denoised_guided(5, fill=True).any()
    assert _bits_equal(r.read_frame(), zero) and _bits_equal(r.read_moments(), zero)
    r.close()


@pytest.mark.parametrize("java_bytes", [True, False])
def test_display_is_the_display_conversion(pt, oracle, renderer_mod, java_bytes):
    r, _ = _open(pt, renderer_mod, "T1")
    r.render_interleaved(1, _seeds(pt, 1, 4), 2, 0, 0)
    F, T = r.read_frame(), r.read_moments()
    for floor in (None, 0.2):
        dn = r.denoise_guided(4, sigma_albedo=INF, albedo_floor=floor, fill=True)
        disp = r.read_display_denoised_guided(4, sigma_albedo=INF, java_bytes=java_bytes, albedo_floor=floor, fill=True)
        assert np.array_equal(disp, oracle.display(dn, 1, java_bytes))
        assert (dn[..., 3] == F[..., 3]).all() and (dn[..., :3][F[..., 3] == 0] != 0).any()
    assert _bits_equal(r.read_frame(), F) and _bits_equal(r.read_moments(), T)
    r.close()


def test_multi_stream_equals_single(pt, renderer_mod):
    out = []
    for kw in ({}, {"devices": [0, 0]}):
        r, _ = _open(pt, renderer_mod, "T1", **kw)
        n = r.render_interleaved(1, _seeds(pt, 1, 3), 2, 1, 1)
        filled, nf = r.fill_frame(albedo_floor=0.2)
        out.append((np.float32([n, nf]), r.read_frame(), r.read_moments(), filled, r.denoise_guided(5, fill=True),
                    r.denoise_guided(5, sigma_albedo=INF, albedo_floor=0.2, fill=True)))
        r.close()
    assert out[0][0][1] > 0
    for a, b in zip(*out):
        assert _bits_equal(a, b)


def test_full_size(pt, renderer_mod):
    """T1 at 1920 x 1080: two frames on the (1, 0) lattice of stride 2; pt_fill_frame against the model over the whole image, the filled count
    exactly; the filtered image against the model on windows (the filter's model of a whole 1080p image takes minutes).  SAFE sigmas: at two
    million pixels no weight may come near the cut (asserted)."""
    w, h = 1920, 1080
    r, _ = _open(pt, renderer_mod, "T1", w, h)
    assert r.render_interleaved(1, _seeds(pt, 1, 2), 2, 1, 0) == w * h // 4
    fr, T, feat = r.read_frame(), r.read_moments(), r.read_features()
    for floor in FLOORS:
        d = _check_fill(r, fr, feat, SAFE, floor)
        assert d["filled"].sum() > 0.6 * w * h
    it, lum_sigma, mf = 3, 2.0, 4
    for floor in FLOORS:
        got = r.denoise_guided(it, lum_sigma, *SAFE, min_frames=mf, albedo_floor=floor if floor else None, fill=True)
        assert np.array_equal(got[..., 3], fr[..., 3])
        compared = 0
        for y0, y1, x0, x1, inner in _windows(w, h):    # its margin of 24 covers the passes' 14, the pooled variance's 3 and the fill's 2
            sub = (slice(y0, y1), slice(x0, x1))
            want = model(fr[sub], feat[sub], T[sub], it, lum_sigma, *SAFE, mf, floor)
            assert np.allclose(got[sub][inner], want[inner], rtol=1e-4, atol=1e-6, equal_nan=True), (floor, y0, x0, np.nanmax(np.abs(got[sub][inner] - want[inner])))
            compared += int(inner.sum())
        assert compared >= 7 * 24 * 64
    assert _bits_equal(r.read_frame(), fr) and _bits_equal(r.read_moments(), T)
    r.close()


def test_demodulated_fill_returns_the_texels(pt, renderer_mod):
    """FRAME = a_p * E * n on the (0, 0) lattice over T1's own features and nothing elsewhere: the illumination is constant, so the demodulated
    fill with the albedo term off gives every filled hit its own texel.  Bound, in units of u = 2^-24: a source's x = fl(fl(a E) / a) is within 2 of
    E; a sum of 24 products carries at most 24 + 1 and S at most 23, so x' is within 51 of E; a_p x', the product with A', the test's division
    by A' and by c's own rounding add 4: 55 u = 3.3e-6, asserted as 4e-6.  The plain fill, told the same, averages the checker's texels."""
    w, h, n, E = 192, 108, 8.0, np.float32(0.6)
    r, _ = _open(pt, renderer_mod, "T1", w, h)
    feat = r.read_features()
    hitp = np.ascontiguousarray(feat[..., 7]).view(np.int32) >= 0
    finite = np.isfinite(feat[..., 0:7]).all(-1)
    a = np.where(hitp[..., None], np.maximum(feat[..., 4:7], np.float32(0.01)), np.float32(1)).astype(np.float32)
    c = np.where(hitp[..., None], a * E, np.float32(0.25)).astype(np.float32)
    on = lattice(h, w, 2, 0, 0)
    fr = np.zeros((h, w, 4), np.float32)
    fr[on] = np.concatenate([c * np.float32(n), np.full((h, w, 1), n, np.float32)], -1)[on]
    r.write_frame(fr)
    got, nf = r.fill_frame(*REAL, albedo_floor=0.01)
    plain, _ = r.fill_frame(*REAL)
    r.close()
    filled = (got[..., 3] > 0) & ~on
    assert nf == int(filled.sum()) and filled.sum() > 0.9 * (finite & ~on).sum()
    rel = np.abs(got[..., :3][filled] / got[..., 3:4][filled] / c[filled] - 1)
    assert rel.max() <= 4e-6, float(rel.max())
    assert np.abs(plain[..., :3][filled] / plain[..., 3:4][filled] / c[filled] - 1).max() > 0.01


# ---------------------------------------------------------------------------------------------------------------- errors

def test_errors_and_unsupported_contexts(pt, renderer_mod):
    PtError = renderer_mod.PtError
    r, _ = _open(pt, renderer_mod, "T1")
    r.render_interleaved(1, _seeds(pt, 1, 2), 2, 0, 0)
    F, T = r.read_frame(), r.read_moments()
    seeds = _seeds(pt, 3, 2)
    bad = [lambda: r.render_interleaved(3, seeds, 0), lambda: r.render_interleaved(3, seeds, 9), lambda: r.render_interleaved(3, seeds, 2, 2, 0),
           lambda: r.render_interleaved(3, seeds, 2, 0, -1), lambda: r.render_interleaved(3, seeds, 1, 1, 0), lambda: r.render_interleaved(3, [], 2),
           lambda: r.fill_frame(0.0), lambda: r.fill_frame(0.3, float("nan")), lambda: r.fill_frame(0.3, 0.05, -1.0)]
    for floor in (-0.01, float("nan"), INF):
        bad += [lambda floor=floor: r.fill_frame(albedo_floor=floor), lambda floor=floor: r.denoise_guided(albedo_floor=floor, fill=True),
                lambda floor=floor: r.read_display_denoised_guided(albedo_floor=floor, fill=True)]
    bad += [lambda: r.denoise_guided(9, fill=True), lambda: r.denoise_guided(2, 0.0, fill=True), lambda: r.denoise_guided(2, min_frames=1, fill=True),
            lambda: r.read_display_denoised_guided(-1, fill=True), lambda: r.denoise_guided(2, sigma_depth=float("nan"), albedo_floor=0.2, fill=True)]
    for call in bad:
        with pytest.raises(PtError) as e:
            call()
        assert e.value.code == -1                       # PT_ERR_ARG
    L, h = r._L, r._h
    n = C.c_int64(7)
    out = np.zeros((H, W, 4), np.float32)
    sd = np.array(seeds, np.int32).ctypes.data
    assert L.pt_render_interleaved(None, 3, 2, sd, 2, 0, 0, None) == -1
    assert L.pt_render_interleaved(h, 3, 2, None, 2, 0, 0, C.byref(n)) == -1 and n.value == 0
    n = C.c_int64(7)
    assert L.pt_fill_frame(None, 0.3, 0.05, 0.1, 0.0, out.ctypes.data, C.byref(n)) == -1 and n.value == 0
    assert L.pt_fill_frame(h, 0.3, 0.05, 0.1, 0.0, None, None) == -1
    assert L.pt_denoise_guided_filled(None, 1, 2.0, 0.3, 0.05, 0.1, 4, 0.0, out.ctypes.data) == -1
    assert L.pt_denoise_guided_filled(h, 1, 2.0, 0.3, 0.05, 0.1, 4, 0.0, None) == -1
    assert L.pt_read_display_denoised_guided_filled(h, 1, 2.0, 0.3, 0.05, 0.1, 4, 0.0, 1, None) == -1
    assert L.pt_fill_frame(h, 0.3, 0.05, 0.1, 0.0, out.ctypes.data, None) == 0          # the count is optional
    assert frames_equal(r.read_frame(), F) and _bits_equal(r.read_moments(), T)      # no failed call touched FRAME or T
    r.close()
    r, wl = _open(pt, renderer_mod, "T1")               # no moments: the filter refuses as the plain one does, the fill does not need them
    r.render_batch(1, _seeds(pt, 1, 2))
    with pytest.raises(PtError) as e:
        r.denoise_guided(fill=True)
    assert e.value.code == -1 and "pt_record_moments" in str(e.value)
    assert r.fill_frame()[1] == 0
    r.close()
    r = renderer_mod.Renderer(W, H)                     # DEBUG != 0: as pt_render_mask
    r.load_workload(wl.with_params(DEBUG=1))
    with pytest.raises(PtError) as e:
        r.render_interleaved(1, seeds)
    assert e.value.code == -5
    r.close()
    for kw in (dict(shard_rank=0, shard_count=2), dict(devices=[0], first_shard=0, total_shards=2)):
        p, _ = _open(pt, renderer_mod, "T1", **kw)
        p.record_moments(True)
        assert 0 < p.render_interleaved(1, _seeds(pt, 1, 2), 2, 0, 0) < W * H // 4      # a part renders its own pixels of the lattice
        Fp = p.read_frame()
        for call in (lambda: p.fill_frame(), lambda: p.denoise_guided(fill=True), lambda: p.read_display_denoised_guided(albedo_floor=0.2, fill=True)):
            with pytest.raises(PtError) as e:
                call()
            assert e.value.code == -5, kw               # PT_ERR_UNSUPPORTED
        assert frames_equal(p.read_frame(), Fp)
        p.close()
