"""GPU: the glare (pt_bloom, pt_tonemap_bloom, pt_tonemap_bloom_save_png; include/pt_bloom.h) against the float32 model of tests/_bloom_model.py
chained with tests/_tonemap_model.py, bit for bit in the floats, the bytes, the exposure and the histogram: the small shapes at which the kernels
take another path (one texel, levels that collapse, odd sizes at every level, exactly the tiles, partial tiles and seams, every special value), a
full-size image, checks that do not rest on the model (intensity 0 and light below the threshold are pt_tonemap; the metering never changes; the
float64 reference's derived bound), the filtered image taken where a filter left it, what the calls leave alone, contexts, the exposure fed
back, the PNG, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import _bloom_model as BM
import _bloom_ref64 as R64
import _tonemap_model as TM
from conftest import frames_equal
from test_gpu_tonemap import _decode_png, _rendered, _same, _seeds, _special_image

pytestmark = pytest.mark.gpu

f32 = np.float32
INF, NAN = float("inf"), float("nan")
DENORM = float(np.finfo(f32).smallest_subnormal)
RULES = [dict(levels=L, spread=s, threshold=t, intensity=0.6) for L in (1, 2, 8) for s in (1.0, 0.5) for t in (0.0, 0.8)]


@pytest.fixture(scope="module")
def T(renderer_mod):
    return renderer_mod.tonemap_srgb_thresholds()


def _lognormal(w, h, seed, counts=True):
    """a log-normal mean image; a is a count 1 .. 6"""
    rs = np.random.RandomState(seed)
    img = np.exp(rs.normal(-0.5, 2.0, (h, w, 4))).astype(f32)
    img[..., 3] = rs.randint(1, 7, (h, w)) if counts else 1.0
    return img


def _as_frame(img):
    """the FRAME whose means are img's: sums under img's own counts (the device divides them again: the means may differ in the last bit)"""
    fr = img.copy()
    with np.errstate(all="ignore"):
        fr[..., :3] = img[..., :3] * img[..., 3:4]
    return fr


def _floats_same(got, want, tag):
    assert got.shape == want.shape and got.dtype == f32
    assert frames_equal(got, want), (tag, "floats", int((~((got == want) | (np.isnan(got) & np.isnan(want)))).any(-1).sum()),
                                     np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:4].tolist())


def _check_both_calls(r, renderer_mod, T, image, c, A, W, H, rules, tag):
    """pt_bloom's floats and pt_tonemap_bloom's bytes, exposure and histogram of `image` (None: FRAME) against the model"""
    for kw in rules:
        br = renderer_mod.bloom_rule(**kw)
        for tm_kw in (dict(), dict(curve=1, transfer=0, exposure=0.37)):
            tm = TM.rule(**tm_kw)
            got = r.tonemap_bloom(image, rule=r.tonemap_rule(**tm), bloom=br, want_hist=True)
            _same(got, BM.tonemap_bloom(c, A, tm, BM.rule(**kw), T, W, H), (tag, kw, tm_kw))
        for e in (1.0, 0.37):
            _floats_same(r.bloom(image, exposure=e, bloom=br), BM.bloom(c, A, W, H, BM.rule(**kw), e), (tag, kw, e))


# ---------------------------------------------------------------------------------------------------------------- small shapes

@pytest.mark.parametrize("W,H", [(1, 1), (2, 1), (1, 7), (5, 3), (33, 17), (64, 64), (70, 37)])
def test_small_shapes_match_the_model(renderer_mod, T, W, H):
    img = _lognormal(W, H, 100 * W + H)
    r = renderer_mod.Renderer(W, H)
    c, A = TM.from_image(img)
    _check_both_calls(r, renderer_mod, T, img, c, A, W, H, RULES, "HOST")
    fr = _as_frame(img)
    assert len(np.unique(fr[..., 3])) > 1 or W * H < 3
    r.write_frame(fr)
    c, A = TM.from_frame(fr)
    _check_both_calls(r, renderer_mod, T, None, c, A, W, H, RULES, "FRAME")
    r.close()


def test_the_special_value_image_matches_the_model_and_its_specials_stay_contained(renderer_mod, T):
    W, H = 50, 27
    img = _special_image(W, H)
    r = renderer_mod.Renderer(W, H)
    c, A = TM.from_image(img)
    _check_both_calls(r, renderer_mod, T, img, c, A, W, H, RULES, "HOST")
    fr = _as_frame(img)
    r.write_frame(fr)
    cF, AF = TM.from_frame(fr)
    _check_both_calls(r, renderer_mod, T, None, cF, AF, W, H, RULES, "FRAME")
    # Contained.  A special pixel is one whose clean value differs from its own: a NaN, a negative or an over-range channel, a count that shows
    # nothing.  Its s is 0 — or 65504 for a channel above that — and nothing else of it reaches a neighbour: every pixel whose source is finite is
    # finite, and equals the model's for the image whose special pixels are replaced by their clean values outright.
    s = BM.clean(c, A)
    special = ~((s == c).all(1) | ((s == 0) & (c == 0)).all(1))
    assert special.sum() > 40 and np.isnan(c).any() and np.isinf(c).any() and (A[special] <= 0).any()
    cleaned = img.copy().reshape(-1, 4)
    cleaned[special, :3] = s[special]
    cleaned[special, 3] = 1.0                                        # (their s already is 0 where the count showed nothing)
    assert np.isfinite(cleaned[:, :3]).all() and (cleaned[:, :3] >= 0).all() and (BM.clean(*TM.from_image(cleaned)) == s).all()
    finite = np.isfinite(c).all(1) & np.isfinite(A)
    assert finite.sum() > W * H // 2 and (special & finite).any()
    for kw in RULES:
        got = r.bloom(img, exposure=0.5, bloom=renderer_mod.bloom_rule(**kw)).reshape(-1, 4)
        assert np.isfinite(got[finite]).all(), kw
        want = r.bloom(cleaned.reshape(H, W, 4), exposure=0.5, bloom=renderer_mod.bloom_rule(**kw)).reshape(-1, 4)
        model = BM.bloom(*TM.from_image(cleaned), W, H, BM.rule(**kw), 0.5).reshape(-1, 4)
        same = finite & ~special                                     # the special pixels' own c differs between the two images; their glare does not
        assert frames_equal(got[same], want[same]) and frames_equal(got[same], model[same]), kw
    r.close()


# ---------------------------------------------------------------------------------------------------------------- full size

def test_full_size_with_impulses_on_the_corners_the_seams_and_a_flat_half(renderer_mod, T):
    W, H = 1920, 1080
    rs = np.random.RandomState(29)
    img = np.empty((H, W, 4), f32)
    img[..., :3] = np.exp(rs.normal(-2.0, 1.0, (H, W, 3)))
    img[..., 3] = 3.0
    img[H // 2:, :, :3] = (0.25, 0.5, 0.125)                         # a flat half
    spots = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]          # the corners
    spots += [(x, y) for x in (31, 32, 33, 1023, 1024) for y in (31, 32, 539, 540)]      # the source tiles' seams (32) and the halves' border
    spots += [(700, 300), (701, 300), (1333, 777), (W - 2, 500), (960, H - 2)]           # the interior and next to the borders
    for k, (x, y) in enumerate(spots):
        img[y, x, :3] = (3000.0 + 100 * k, 500.0 * (k % 3), 40000.0 if k % 5 == 0 else 10.0)
    c, A = TM.from_image(img)
    kw = dict(levels=6, spread=0.75, threshold=1.0, intensity=0.05)
    tm = TM.rule()
    r = renderer_mod.Renderer(W, H)
    br = renderer_mod.bloom_rule(**kw)
    got = r.tonemap_bloom(img, rule=r.tonemap_rule(**tm), bloom=br, want_hist=True)
    want = BM.tonemap_bloom(c, A, tm, BM.rule(**kw), T, W, H)
    _same(got, want, "1080p")
    plain = r.tonemap(img, rule=r.tonemap_rule(**tm))
    assert got[1] == plain[1] and (got[0] != plain[0]).any(-1).sum() > 10000      # the glare shows, the exposure is the source's
    _floats_same(r.bloom(img, exposure=float(want[1]), bloom=br), BM.bloom(c, A, W, H, BM.rule(**kw), want[1]), "1080p")
    r.close()


# ---------------------------------------------------------------------------------------------------------------- not resting on the model

def test_intensity_0_and_light_below_the_threshold_are_pt_tonemap(pt, renderer_mod):
    r = _rendered(pt, renderer_mod)                                   # a-trous needs no moments
    img = _lognormal(48, 27, 41)
    X = r.denoise()
    sources = ((None, None), (img, img), ("filtered", X))
    for src, plain_src in sources:
        if isinstance(src, str):
            r.denoise()
        for tm_kw in (dict(), dict(curve=1, transfer=0, adapt=0.5)):
            tm = r.tonemap_rule(**tm_kw)
            plain = r.tonemap(plain_src, prev_exposure=2.0, rule=tm, want_hist=True)
            for kw in (dict(intensity=0.0), dict(intensity=0.0, levels=1, threshold=0.0, spread=1.0), dict(intensity=0.0, levels=8, threshold=0.0, spread=0.5)):
                _same(r.tonemap_bloom(src, prev_exposure=2.0, rule=tm, bloom=r.bloom_rule(**kw), want_hist=True), plain, ("intensity 0", kw))
            # for any bloom rule the exposure and the histogram are pt_tonemap's
            for kw in (dict(intensity=5.0, threshold=0.0), dict(levels=1, intensity=0.5), dict(levels=8, spread=0.1, intensity=1e6)):
                rgb, e, hist = r.tonemap_bloom(src, prev_exposure=2.0, rule=tm, bloom=r.bloom_rule(**kw), want_hist=True)
                assert f32(e).view(np.uint32) == f32(plain[1]).view(np.uint32) and np.array_equal(hist, plain[2]), kw
    # every pixel's exposed luminance at or below the threshold: nothing blooms, whatever the intensity
    dim = _lognormal(48, 27, 43)
    dim[..., :3] = np.minimum(dim[..., :3], f32(1.9))                # l <= 1.9 * (0.2126 + 0.7152 + 0.0722) < 1.95;  l * 0.5 < threshold 1
    dim[3, 4, :3] = 0.0
    tm = r.tonemap_rule(exposure=0.5)
    assert (TM.luminance(TM.from_image(dim)[0]) * f32(0.5) <= 1.0).all()
    plain = r.tonemap(dim, rule=tm, want_hist=True)
    for kw in (dict(intensity=3.0, threshold=1.0), dict(intensity=1e30, threshold=1.0, levels=8, spread=1.0)):
        _same(r.tonemap_bloom(dim, rule=tm, bloom=r.bloom_rule(**kw), want_hist=True), plain, ("below the threshold", kw))
    lit = r.tonemap_bloom(dim, rule=tm, bloom=r.bloom_rule(intensity=3.0, threshold=0.5))[0]
    assert (lit != plain[0]).any()                                   # and above it something does
    r.close()


@pytest.mark.parametrize("W,H,L,spread,thr", [(70, 37, 8, 0.5, 0.0), (64, 64, 6, 1.0, 1.0), (33, 17, 2, 0.75, 0.3), (5, 3, 8, 1.0, 0.0), (1, 1, 1, 1.0, 0.0)])
def test_the_floats_are_within_the_derived_bound_of_the_float64_reference(renderer_mod, W, H, L, spread, thr):
    img = _lognormal(W, H, 7 * W + H + L)
    img[..., 3][::3, ::2] = 0.0                                       # some pixels emit nothing
    c, A = TM.from_image(img)
    r = renderer_mod.Renderer(W, H)
    kw = dict(levels=L, spread=spread, threshold=thr, intensity=0.7)
    for e in (1.0, 0.37):
        got = r.bloom(img, exposure=e, bloom=renderer_mod.bloom_rule(**kw))
        ref, bound = R64.bloom(c, A, W, H, BM.rule(**kw), BM.threshold(thr, e))
        err = np.abs(got[..., :3].astype(np.float64) - ref[..., :3])
        assert (err <= bound).all(), (float((err / bound).max()), np.argwhere(err > bound)[:4].tolist())      # no pixel excluded
        assert np.array_equal(got[..., 3], img[..., 3])
    r.close()


# ---------------------------------------------------------------------------------------------------------------- the filtered source

def _refused_filtered(r):
    L = r._L
    tm, bl = r.tonemap_rule(), r.bloom_rule()
    rgb, hist, e = np.full(r.W * r.H * 3, 9, np.uint8), np.full(512, 5, np.uint32), C.c_float(7.0)
    rc = L.pt_tonemap_bloom(r._h, C.byref(tm), C.byref(bl), 2, None, 0.0, rgb.ctypes.data, C.byref(e), hist.ctypes.data)
    text = L.pt_last_error().decode()
    assert rc == -1 and text.startswith("pt_tonemap_bloom: no filtered image on the device"), (rc, text)
    assert (rgb == 9).all() and (hist == 5).all() and e.value == 7.0
    rgba = np.full(r.W * r.H * 4, 3.0, f32)
    assert L.pt_bloom(r._h, C.byref(bl), 2, None, 1.0, rgba.ctypes.data) == -1 and L.pt_last_error().decode().startswith("pt_bloom: no filtered image")
    assert (rgba == 3.0).all()


def test_the_filtered_image_is_taken_where_the_filter_left_it(pt, renderer_mod):
    for devices in (None, [0, 0]):
        r = _rendered(pt, renderer_mod, frames=4, moments=True, **({} if devices is None else {"devices": devices}))
        _refused_filtered(r)                                          # before any filter call
        br = r.bloom_rule(levels=4, intensity=0.4, threshold=0.2)

        def same_as(X, tag):
            for call in (lambda s: r.tonemap_bloom(s, bloom=br, want_hist=True), lambda s: r.tonemap_bloom(s, rule=r.tonemap_rule(exposure=1.5, curve=1), bloom=br, want_hist=True)):
                _same(call("filtered"), call(X), (devices, tag))
            _floats_same(r.bloom("filtered", exposure=0.8, bloom=br), r.bloom(X, exposure=0.8, bloom=br), (devices, tag))
        X = r.denoise_guided(iterations=3)
        assert np.isfinite(X).all() and X[..., :3].max() > 0
        same_as(X, "denoise_guided")
        same_as(X, "read only: a second time")                        # the calls left the filtered image as it was
        Y = r.denoise(iterations=2)
        assert not frames_equal(X, Y)
        same_as(Y, "denoise")
        r.read_display_denoised_guided(iterations=3)                  # X again, delivered as bytes: the floats stay on the device
        same_as(X, "read_display_denoised_guided")
        r.select_guided(0.05)                                         # T is there: the selection does not touch the filtered image
        same_as(X, "after a selection with moments")
        r.close()
    # without moments the selection zeroes that buffer as its stand-in for T: the filtered image is gone until the next filter call
    r = _rendered(pt, renderer_mod)
    _refused_filtered(r)
    Y = r.denoise(iterations=2)
    _same(r.tonemap_bloom("filtered", bloom=br, want_hist=True), r.tonemap_bloom(Y, bloom=br, want_hist=True), "denoise")
    r.select_guided(0.05)
    _refused_filtered(r)
    with pytest.raises(renderer_mod.PtError) as err:
        r.tonemap_bloom("filtered")
    assert err.value.code == -1
    r.read_display_denoised(iterations=2)                             # a later filter call makes it available again
    _same(r.tonemap_bloom("filtered", bloom=br, want_hist=True), r.tonemap_bloom(Y, bloom=br, want_hist=True), "read_display_denoised")
    r.close()


# ---------------------------------------------------------------------------------------------------------------- state, contexts, metering

def test_the_calls_are_read_only(pt, renderer_mod, tmp_path):
    r = _rendered(pt, renderer_mod, moments=True)
    twin = _rendered(pt, renderer_mod, moments=True)
    before = r.read_frame(), r.read_moments(), r.read_features()
    X = r.denoise_guided(iterations=2)
    img = np.ones((27, 48, 4), f32)
    for image in (None, img, "filtered"):
        r.tonemap_bloom(image, want_hist=True)
        r.tonemap_bloom(image, rule=r.tonemap_rule(exposure=1.5, curve=1, transfer=0), bloom=r.bloom_rule(levels=8, spread=1.0))
        r.bloom(image, exposure=2.0)
        r.tonemap_bloom_save_png(tmp_path / "x.png", image)
    assert frames_equal(r.read_frame(), before[0]) and frames_equal(r.read_moments(), before[1]) and frames_equal(r.read_features(), before[2])
    assert frames_equal(r.denoise_guided(iterations=2), X)
    twin.denoise_guided(iterations=2)
    for q in (r, twin):
        q.render_batch(3, _seeds(pt, 3, 2))
    assert frames_equal(r.read_frame(), twin.read_frame()) and frames_equal(r.read_moments(), twin.read_moments())
    r.close()
    twin.close()


def test_a_multi_stream_context_equals_one_stream(pt, renderer_mod, T):
    img = _special_image(48, 27, seed=3)

    def sequence(**kw):
        r = _rendered(pt, renderer_mod, **kw)
        br = r.bloom_rule(levels=5, intensity=0.5, threshold=0.1)
        out = (r.tonemap_bloom(bloom=br, want_hist=True), r.tonemap_bloom(img, bloom=br, want_hist=True),
               r.tonemap_bloom(rule=r.tonemap_rule(curve=1, transfer=0, adapt=0.5), bloom=br, prev_exposure=3.0, want_hist=True))
        floats = r.bloom(exposure=0.7, bloom=br), r.bloom(img, exposure=0.7, bloom=br)
        frame = r.read_frame()
        r.close()
        return out, floats, frame
    one, floats, frame = sequence()
    c, A = TM.from_frame(frame)
    kw = dict(levels=5, intensity=0.5, threshold=0.1, spread=BM.RULE["spread"])
    _same(one[0], BM.tonemap_bloom(c, A, TM.rule(), kw, T, 48, 27), "one stream")
    _floats_same(floats[0], BM.bloom(c, A, 48, 27, kw, 0.7), "one stream")
    for ctx in ({"devices": [0, 0]}, {"devices": [0]}):
        got, gfloats, f2 = sequence(**ctx)
        assert frames_equal(f2, frame)
        for a, b in zip(got, one):
            _same(a, b, ctx)
        for a, b in zip(gfloats, floats):
            _floats_same(a, b, ctx)


def test_a_part_of_the_image_is_refused(pt, renderer_mod):
    wl = pt.scenes.build("C2", 48, 27)
    img = np.ones((27, 48, 4), f32)
    for kw in ({"shard_rank": 0, "shard_count": 2}, {"devices": [0], "first_shard": 0, "total_shards": 2}):
        q = renderer_mod.Renderer(48, 27, **kw)
        q.load_workload(wl)
        q.reset_frame()
        q.render_batch(1, _seeds(pt, 1, 2))
        before = q.read_frame()
        tm, bl = q.tonemap_rule(), q.bloom_rule()
        for source, image in ((0, None), (1, img), (2, None)):
            ptr = None if image is None else image.ctypes.data
            rgb, hist, e, rgba = np.full(48 * 27 * 3, 9, np.uint8), np.full(512, 5, np.uint32), C.c_float(7.0), np.full(48 * 27 * 4, 3.0, f32)
            rc = q._L.pt_tonemap_bloom(q._h, C.byref(tm), C.byref(bl), source, ptr, 0.0, rgb.ctypes.data, C.byref(e), hist.ctypes.data)
            assert rc == -5 and b"pt_tonemap_bloom needs the whole image" in q._L.pt_last_error(), (kw, rc)      # PT_ERR_UNSUPPORTED
            rc = q._L.pt_bloom(q._h, C.byref(bl), source, ptr, 1.0, rgba.ctypes.data)
            assert rc == -5 and b"pt_bloom needs the whole image" in q._L.pt_last_error(), (kw, rc)
            assert (rgb == 9).all() and (hist == 5).all() and e.value == 7.0 and (rgba == 3.0).all()
        with pytest.raises(renderer_mod.PtError) as err:
            q.tonemap_bloom()
        assert err.value.code == -5
        assert frames_equal(q.read_frame(), before), kw
        q.close()


def test_three_steps_with_the_exposure_fed_back_equal_the_models_sequence(renderer_mod, T):
    W, H = 50, 27
    rs = np.random.RandomState(31)
    images = [np.concatenate([np.exp(rs.normal(mu, 1.5, (H, W, 3))), np.ones((H, W, 1))], -1).astype(f32) for mu in (-2.0, 1.5, 4.0)]
    tm = TM.rule(adapt=0.3)
    kw = dict(levels=4, intensity=0.3, threshold=1.0, spread=0.6)
    r = renderer_mod.Renderer(W, H)
    prev = wprev = 0.0
    for k, img in enumerate(images):
        got = r.tonemap_bloom(img, prev_exposure=prev, rule=r.tonemap_rule(**tm), bloom=r.bloom_rule(**kw), want_hist=True)
        c, A = TM.from_image(img)
        want = BM.tonemap_bloom(c, A, tm, BM.rule(**kw), T, W, H, prev=wprev)
        _same(got, want, k)
        assert (got[0] != r.tonemap(img, prev_exposure=prev, rule=r.tonemap_rule(**tm))[0]).any()      # the threshold follows the exposure: each step blooms
        prev, wprev = got[1], want[1]
    r.close()


# ---------------------------------------------------------------------------------------------------------------- the PNG and the refusals

def test_the_png_decodes_to_the_bytes(pt, renderer_mod, tmp_path):
    img = _special_image(48, 27, seed=5)
    for kw in (dict(), dict(devices=[0, 0])):
        r = _rendered(pt, renderer_mod, **kw)
        r.denoise(iterations=2)
        br = r.bloom_rule(intensity=0.5, threshold=0.1)
        for k, image in enumerate((None, img, "filtered")):
            path = tmp_path / f"bl_{k}.png"
            e = r.tonemap_bloom_save_png(path, image, prev_exposure=2.0, rule=r.tonemap_rule(adapt=0.5), bloom=br)
            rgb, e2 = r.tonemap_bloom(image, prev_exposure=2.0, rule=r.tonemap_rule(adapt=0.5), bloom=br)
            w, h, got = _decode_png(path.read_bytes())
            assert (w, h) == (48, 27) and np.array_equal(got, rgb) and e == e2 and rgb.max() > 0
        r.close()


def test_every_refusal_leaves_the_outputs_as_they_were(pt, renderer_mod, tmp_path):
    r = _rendered(pt, renderer_mod)
    L = r._L
    img = np.ones((27, 48, 4), f32)
    before = r.read_frame()

    def refused(tm, bl, source=0, image=None, prev=0.0, exposure=1.0, display=True, floats=True, code=-1):
        ptr = None if image is None else image.ctypes.data
        tmp, blp = (None if tm is None else C.byref(tm)), (None if bl is None else C.byref(bl))
        texts = []
        if display:
            rgb, hist, e = np.full(48 * 27 * 3, 9, np.uint8), np.full(512, 5, np.uint32), C.c_float(7.0)
            rc = L.pt_tonemap_bloom(r._h, tmp, blp, source, ptr, prev, rgb.ctypes.data, C.byref(e), hist.ctypes.data)
            texts.append(L.pt_last_error().decode())
            assert rc == code and texts[-1].startswith("pt_tonemap_bloom: "), (rc, texts)
            assert (rgb == 9).all() and (hist == 5).all() and e.value == 7.0, texts
            rc = L.pt_tonemap_bloom_save_png(r._h, tmp, blp, source, ptr, prev, str(tmp_path / "never.png").encode(), C.byref(e))
            assert rc == code and L.pt_last_error().decode() == texts[-1].replace("pt_tonemap_bloom: ", "pt_tonemap_bloom_save_png: ") and e.value == 7.0
            assert not (tmp_path / "never.png").exists()
        if floats:
            rgba = np.full(48 * 27 * 4, 3.0, f32)
            rc = L.pt_bloom(r._h, blp, source, ptr, exposure, rgba.ctypes.data)
            texts.append(L.pt_last_error().decode())
            assert rc == code and texts[-1].startswith("pt_bloom: ") and (rgba == 3.0).all(), (rc, texts)
        return " | ".join(texts)

    tm, bl = r.tonemap_rule(), r.bloom_rule()
    assert "null rule" in refused(None, bl, floats=False) and "null bloom rule" in refused(tm, None)
    bad_tm = dict(curve=(-1, 3), transfer=(2,), exposure=(-1.0, NAN), key=(0.0, INF), lo_pct=(-0.1, NAN), hi_pct=(0.05, 1.5), min_exposure=(0.0, NAN),
                  max_exposure=(2.0 ** -11, INF), white=(0.0, NAN), adapt=(0.0, 1.5))
    for name, values in bad_tm.items():
        for v in values:
            assert "rule." + name in refused(r.tonemap_rule(**{name: v}), bl, floats=False), (name, v)
    bad_bl = dict(levels=(0, 9, -1), intensity=(-1.0, -DENORM, INF, NAN), threshold=(-1.0, INF, -INF, NAN), spread=(0.0, -0.5, 1.5, INF, NAN))
    for name, values in bad_bl.items():
        for v in values:
            for source, image in ((0, None), (1, img)):
                text = refused(tm, r.bloom_rule(**{name: v}), source=source, image=image)
                assert text.count("bloom." + name) == 2, (name, v, text)
    for prev in (-1.0, INF, NAN):
        assert "prev_exposure" in refused(tm, bl, prev=prev, floats=False)
    for source in (-1, 3, 7):
        assert refused(tm, bl, source=source).count("source must be") == 2
    assert refused(tm, bl, source=0, image=img).count("rgba_in must be NULL") == 2
    assert refused(tm, bl, source=2, image=img).count("rgba_in must be NULL") == 2
    assert refused(tm, bl, source=1, image=None).count("needs rgba_in") == 2
    for e in (0.0, -1.0, INF, NAN):
        assert "exposure must be finite and > 0" in refused(tm, bl, exposure=e, display=False)
    # the order: the tone-map rule, prev_exposure, then the bloom rule in its struct's order, the source, the image; pt_bloom's exposure last
    assert "rule.curve" in refused(r.tonemap_rule(curve=7), r.bloom_rule(levels=0), source=9, prev=-1.0, floats=False)
    assert "prev_exposure" in refused(tm, r.bloom_rule(levels=0), source=9, prev=-1.0, floats=False)
    assert refused(tm, r.bloom_rule(levels=0, spread=2.0), source=9, exposure=NAN).count("bloom.levels") == 2
    assert refused(tm, r.bloom_rule(spread=2.0), source=9, exposure=NAN).count("bloom.spread") == 2
    assert refused(tm, bl, source=9, image=img, exposure=NAN).count("source must be") == 2
    assert "rgba_in must be NULL" in refused(tm, bl, source=0, image=img, exposure=NAN, display=False)
    assert refused(tm, bl, source=2).count("no filtered image on the device") == 2      # no filter call was made
    # the PNG's own: a null path, a file that cannot be written
    e = C.c_float(7.0)
    assert L.pt_tonemap_bloom_save_png(r._h, C.byref(tm), C.byref(bl), 0, None, 0.0, None, C.byref(e)) == -1
    assert L.pt_last_error() == b"pt_tonemap_bloom_save_png: null argument"
    nowhere = str(tmp_path / "no_such_directory" / "x.png").encode()
    assert L.pt_tonemap_bloom_save_png(r._h, C.byref(tm), C.byref(bl), 0, None, 0.0, nowhere, C.byref(e)) == -1
    assert L.pt_last_error() == b"pt_tonemap_bloom_save_png: cannot open " + nowhere and e.value == 7.0
    # a null context, with a device in the process; every output is optional, and the calls still go through
    assert L.pt_tonemap_bloom(None, C.byref(tm), C.byref(bl), 0, None, 0.0, None, C.byref(e), None) == -1 and e.value == 7.0
    assert L.pt_tonemap_bloom(r._h, C.byref(tm), C.byref(bl), 0, None, 0.0, None, None, None) == 0
    assert L.pt_tonemap_bloom(r._h, C.byref(tm), C.byref(bl), 0, None, 0.0, None, C.byref(e), None) == 0 and e.value == r.tonemap()[1] != 7.0
    assert L.pt_bloom(r._h, C.byref(bl), 0, None, 1.0, None) == 0
    assert frames_equal(r.read_frame(), before)
    r.close()
