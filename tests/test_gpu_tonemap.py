"""GPU: the display image (pt_tonemap, pt_tonemap_save_png; include/pt_tonemap.h) against the float32 model of tests/_tonemap_model.py, bit for
bit in the bytes, the exposure and the histogram: injected images with every special value, luminances on both sides of the bin edges,
channels on both sides of every code edge, a full-size image with a flat half, the FRAME path (rendered, and written with differing counts),
what the call leaves alone, contexts, the damped exposure fed back, the PNG, and every refusal."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import _tonemap_model as TM
from conftest import frames_equal

pytestmark = pytest.mark.gpu

f32 = np.float32
INF, NAN = float("inf"), float("nan")
DENORM = float(np.finfo(f32).smallest_subnormal)
MODES = [(curve, transfer) for curve in (0, 1, 2) for transfer in (0, 1)]


@pytest.fixture(scope="module")
def T(renderer_mod):
    return renderer_mod.tonemap_srgb_thresholds()


def _seeds(pt, first, n):
    return [pt.scenes.frame_seed(f) for f in range(first, first + n)]


def _same(got, want, tag):
    """(bytes, exposure, histogram) of the device against the model's"""
    rgb, e, hist = got
    wrgb, we, whist = want
    assert np.array_equal(hist, whist), (tag, "histogram", np.flatnonzero(hist != whist)[:8], int(hist.sum()), int(whist.sum()))
    assert f32(e).view(np.uint32) == f32(we).view(np.uint32), (tag, "exposure", e, float(we))
    assert rgb.shape == wrgb.shape and rgb.dtype == np.uint8
    assert np.array_equal(rgb, wrgb), (tag, "bytes", int((rgb != wrgb).any(-1).sum()), np.argwhere((rgb != wrgb).any(-1))[:4].tolist())


def _special_image(w, h, seed=7):
    """a log-normal image with every value the rule has a branch for; a is a count (1 .. 6) with the special ones among them"""
    rs = np.random.RandomState(seed)
    img = np.exp(rs.normal(-1.0, 2.5, (h, w, 4))).astype(f32)
    img[..., 3] = rs.randint(1, 7, (h, w))
    spots = [(y, x) for y in range(h) for x in range(w)]
    rs.shuffle(spots)
    it = iter(spots)

    def put(rgb=None, a=None, ch=None, v=None):
        y, x = next(it)
        if rgb is not None:
            img[y, x, :3] = rgb
        if ch is not None:
            img[y, x, ch] = v
        if a is not None:
            img[y, x, 3] = a
    for v in (NAN, INF, -INF, -0.5, 0.0, -0.0, DENORM, -DENORM, 1e-40, 65504.0, 65505.0, 3e38):      # in one component, and in all three
        for ch in (0, 1, 2):
            put(ch=ch, v=v)
        put(rgb=(v, v, v))
    for a in (0.0, -0.0, -1.0, NAN, INF, -INF, 0.5, DENORM):                                         # counts
        put(a=a)
        put(a=a, rgb=(0.5, 2.0, 8.0))
    for l in (2.0 ** -17, 2.0 ** -16, 1e-30, DENORM, 2.0 ** 16, 2.0 ** 17, 1e30, 3e38):               # luminances outside the bins' range
        put(rgb=(l, l, l), a=1.0)
    put(rgb=(INF, -INF, 1.0))                                                                        # a NaN luminance from finite-free parts
    put(rgb=(-1.0, 0.25, 0.0))                                                                       # negative and positive: l = 0 or near it
    put(rgb=(-3e38, 3e38, 3e38))
    return img


# ---------------------------------------------------------------------------------------------------------------- injected images

def test_a_small_image_with_every_special_value_matches_the_model(renderer_mod, T):
    W, H = 50, 27                                       # W no multiple of 4 or 64, H odd, 1350 pixels: five full blocks and a partial one
    img = _special_image(W, H)
    c, A = TM.from_image(img)
    assert TM.metered(c, A).sum() > W * H // 2 and (~TM.metered(c, A)).sum() > 25
    h = TM.histogram(c, A)
    assert h[0] >= 4 and h[511] >= 4 and np.isnan(TM.luminance(c)).any()
    r = renderer_mod.Renderer(W, H)
    for curve, transfer in MODES:
        for fixed in (0.0, 0.37):
            for white in ((4.0, 1e-30) if curve == 1 else (4.0,)):      # white*white underflows to 0: x/0 and 0/0 in the curve
                rule = TM.rule(curve=curve, transfer=transfer, exposure=fixed, white=white)
                got = r.tonemap(img, rule=r.tonemap_rule(**rule), want_hist=True)
                _same(got, TM.tonemap(c, A, rule, T, W, H), (curve, transfer, fixed, white))
    # the histogram is optional, and skipped under a fixed exposure it changes nothing
    rule = TM.rule(exposure=0.37)
    rgb, e = r.tonemap(img, rule=r.tonemap_rule(**rule))
    assert e == f32(0.37) and np.array_equal(rgb, TM.apply(c, A, f32(0.37), rule, T, W, H))
    # the same pixels as a FRAME: sums and their own counts
    fr = img.copy()
    with np.errstate(all="ignore"):
        fr[..., :3] = img[..., :3] * img[..., 3:4]
    r.write_frame(fr)
    cF, AF = TM.from_frame(fr)
    for curve, transfer in MODES:
        rule = TM.rule(curve=curve, transfer=transfer, lo_pct=0.0, hi_pct=1.0)
        _same(r.tonemap(rule=r.tonemap_rule(**rule), want_hist=True), TM.tonemap(cF, AF, rule, T, W, H), ("FRAME", curve, transfer))
    r.close()


def _edge_colours():
    """(red, green) pairs whose luminance (0.2126*r + 0.7152*g) + 0 lands on the first float of bin b and on the last float below it, for
    every edge b-1 | b found: green near L / 0.7152, and a little red, a few ulps of L, to reach the floats that green's steps skip"""
    out = {}
    for b in range(1, TM.BINS):
        first = np.array([(b + 1776) << 19], np.uint32).view(f32)[0]
        last = np.nextafter(first, f32(0))
        found = []
        for want in (last, first):
            cand = np.array([f32(float(want) / 0.7152)], f32)
            for _ in range(6):
                cand = np.unique(np.concatenate([cand, np.nextafter(cand, f32(0)), np.nextafter(cand, f32(INF))]))
            red = (np.arange(0, 12, dtype=f32) * np.spacing(want)).astype(f32)
            c = np.zeros((cand.size, red.size, 3), f32)
            c[..., 1] = cand[:, None]
            c[..., 0] = red[None, :]
            c = c.reshape(-1, 3)
            hit = np.flatnonzero(TM.luminance(c).view(np.uint32) == want.view(np.uint32))
            if hit.size:
                found.append((c[hit[0], 0], c[hit[0], 1]))
        if len(found) == 2:
            out[b] = found
    return out


def test_luminances_on_both_sides_of_the_bin_edges(renderer_mod, T):
    edges = _edge_colours()
    assert len(edges) >= 64 and 1 in edges and 511 in edges, len(edges)        # 0 | 1 and 510 | 511 among them
    W = 37
    H = (2 * len(edges) + W - 1) // W
    img = np.zeros((H * W, 4), f32)                                              # the padding is black: not metered
    want_hist = np.zeros(TM.BINS, np.int64)
    for k, (b, (below, at)) in enumerate(sorted(edges.items())):
        img[2 * k] = (below[0], below[1], 0.0, 1.0)
        img[2 * k + 1] = (at[0], at[1], 0.0, 1.0)
        want_hist[b - 1] += 1
        want_hist[b] += 1
    c, A = TM.from_image(img)
    assert np.array_equal(TM.histogram(c, A), want_hist)                         # the model puts each pair across its edge
    r = renderer_mod.Renderer(W, H)
    rule = TM.rule()
    got = r.tonemap(img, rule=r.tonemap_rule(**rule), want_hist=True)
    assert np.array_equal(got[2], want_hist)
    _same(got, TM.tonemap(c, A, rule, T, W, H), "bin edges")
    r.close()


def test_channels_on_both_sides_of_every_code_edge(renderer_mod, T):
    one = f32(1.0)
    # transfer 1: T[k] and the float below it;  transfer 0: the first float whose t*255 + 0.5 reaches k, and the float below it
    lin = []
    for k in range(1, 256):
        t = f32((k - 0.5) / 255.0)
        while np.floor(t * f32(255.0) + f32(0.5)) >= k:
            t = np.nextafter(t, f32(-1))
        while np.floor(t * f32(255.0) + f32(0.5)) < k:
            t = np.nextafter(t, f32(2))
        lin.append(t)
    lin = np.array(lin, f32)
    for transfer, at in ((1, T[1:]), (0, lin)):
        vals = np.stack([at, np.nextafter(at, f32(-1))], 1).ravel()              # k = 1: (T[1], below), k = 2: ...
        want = np.stack([np.arange(1, 256), np.arange(0, 255)], 1).ravel().astype(np.uint8)
        assert np.array_equal(TM.codes(vals, transfer, T), want)
        W, H = 17, 10                                                            # 170 pixels = 510 channels
        img = np.concatenate([vals.reshape(-1, 3), np.ones((170, 1), f32)], 1).astype(f32)
        r = renderer_mod.Renderer(W, H)
        rgb, e = r.tonemap(img, rule=r.tonemap_rule(curve=0, transfer=transfer, exposure=1.0))
        assert e == one
        assert np.array_equal(rgb, want.reshape(H, W, 3)[::-1]), (transfer, np.argwhere(rgb != want.reshape(H, W, 3)[::-1])[:4].tolist())
        r.close()


def test_full_size_with_a_flat_half(renderer_mod, T):
    W, H = 1920, 1080
    rs = np.random.RandomState(19)
    img = np.empty((H, W, 4), f32)
    img[..., :3] = np.exp(rs.normal(-1.0, 2.0, (H, W, 3)))
    img[..., 3] = 4.0
    img[H // 2:, :, :3] = (0.25, 0.5, 0.125)                                     # a flat half: whole waves in one bin
    img[5, 7, 3] = 0.0
    c, A = TM.from_image(img)
    rule = TM.rule()
    want = TM.tonemap(c, A, rule, T, W, H)
    assert np.array_equal(want[2], np.bincount(TM.bin_of(TM.luminance(c))[TM.metered(c, A)], minlength=TM.BINS))
    assert want[2].max() >= W * (H // 2) and want[2].sum() == W * H - 1 and (want[2] > 0).sum() > 100
    r = renderer_mod.Renderer(W, H)
    _same(r.tonemap(img, rule=r.tonemap_rule(**rule), want_hist=True), want, "1080p")
    r.close()


# ---------------------------------------------------------------------------------------------------------------- the FRAME path

def _rendered(pt, renderer_mod, scene="C2", w=48, h=27, frames=2, moments=False, **kw):
    wl = pt.scenes.build(scene, w, h)
    r = renderer_mod.Renderer(w, h, **kw)
    r.load_workload(wl)
    if moments:
        r.record_moments(True)
    r.reset_frame()
    r.render_batch(1, _seeds(pt, 1, frames))
    return r


def test_a_rendered_frame_matches_the_model(pt, renderer_mod, T):
    r = _rendered(pt, renderer_mod)
    c, A = TM.from_frame(r.read_frame())
    for kw in (dict(), dict(curve=1, transfer=0), dict(curve=0, exposure=2.0)):
        rule = TM.rule(**kw)
        _same(r.tonemap(rule=r.tonemap_rule(**rule), want_hist=True), TM.tonemap(c, A, rule, T, 48, 27), kw)
    r.close()


def test_a_written_frame_with_differing_and_zero_counts_matches_the_model(renderer_mod, T):
    W, H = 50, 27
    rs = np.random.RandomState(23)
    fr = np.exp(rs.normal(0.0, 1.5, (H, W, 4))).astype(f32)
    fr[..., 3] = rs.randint(0, 9, (H, W))                                        # one pixel in nine was never rendered
    fr[..., :3] *= fr[..., 3:4]
    assert (fr[..., 3] == 0).sum() > 50 and len(np.unique(fr[..., 3])) == 9
    r = renderer_mod.Renderer(W, H)
    r.write_frame(fr)
    c, A = TM.from_frame(fr)
    for curve, transfer in MODES:
        rule = TM.rule(curve=curve, transfer=transfer)
        got = r.tonemap(rule=r.tonemap_rule(**rule), want_hist=True)
        _same(got, TM.tonemap(c, A, rule, T, W, H), (curve, transfer))
        assert (got[0][::-1][fr[..., 3] == 0] == 0).all()                        # a count of 0 is black
    r.close()


def test_the_call_is_read_only(pt, renderer_mod, T):
    r = _rendered(pt, renderer_mod, moments=True)
    twin = _rendered(pt, renderer_mod, moments=True)
    before = r.read_frame(), r.read_moments()
    img = np.ones((27, 48, 4), f32)
    for image in (None, img):
        r.tonemap(image, want_hist=True)
        r.tonemap(image, rule=r.tonemap_rule(exposure=1.5, curve=1, transfer=0))
    assert frames_equal(r.read_frame(), before[0]) and frames_equal(r.read_moments(), before[1])
    for q in (r, twin):
        q.render_batch(3, _seeds(pt, 3, 2))
    assert frames_equal(r.read_frame(), twin.read_frame()) and frames_equal(r.read_moments(), twin.read_moments())
    r.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------- contexts

def test_a_multi_stream_context_equals_one_stream(pt, renderer_mod, T):
    img = _special_image(48, 27, seed=3)

    def sequence(**kw):
        r = _rendered(pt, renderer_mod, **kw)
        out = r.tonemap(want_hist=True), r.tonemap(img, want_hist=True), r.tonemap(rule=r.tonemap_rule(curve=1, transfer=0, adapt=0.5), prev_exposure=3.0, want_hist=True)
        frame = r.read_frame()
        r.close()
        return out, frame
    one, frame = sequence()
    c, A = TM.from_frame(frame)
    _same(one[0], TM.tonemap(c, A, TM.rule(), T, 48, 27), "one stream")
    for kw in ({"devices": [0, 0]}, {"devices": [0]}):
        got, f2 = sequence(**kw)
        assert frames_equal(f2, frame)
        for a, b in zip(got, one):
            _same(a, b, kw)


def test_a_part_of_the_image_is_refused(pt, renderer_mod):
    wl = pt.scenes.build("C2", 48, 27)
    img = np.ones((27, 48, 4), f32)
    for kw in ({"shard_rank": 0, "shard_count": 2}, {"devices": [0], "first_shard": 0, "total_shards": 2}):
        q = renderer_mod.Renderer(48, 27, **kw)
        q.load_workload(wl)
        q.reset_frame()
        q.render_batch(1, _seeds(pt, 1, 2))
        before = q.read_frame()
        rule = q.tonemap_rule()
        for image in (None, img):
            rgb, hist, e = np.full(48 * 27 * 3, 9, np.uint8), np.full(512, 5, np.uint32), C.c_float(7.0)
            rc = q._L.pt_tonemap(q._h, C.byref(rule), None if image is None else image.ctypes.data, 0.0, rgb.ctypes.data, C.byref(e), hist.ctypes.data)
            assert rc == -5 and b"pt_tonemap needs the whole image" in q._L.pt_last_error(), (kw, rc)      # PT_ERR_UNSUPPORTED
            assert (rgb == 9).all() and (hist == 5).all() and e.value == 7.0
        with pytest.raises(renderer_mod.PtError) as err:
            q.tonemap()
        assert err.value.code == -5
        assert frames_equal(q.read_frame(), before), kw
        q.close()


# ---------------------------------------------------------------------------------------------------------------- the exposure fed back

def test_three_steps_with_the_exposure_fed_back_equal_the_models_sequence(renderer_mod, T):
    W, H = 50, 27
    rs = np.random.RandomState(31)
    images = [np.concatenate([np.exp(rs.normal(mu, 1.0, (H, W, 3))), np.ones((H, W, 1))], -1).astype(f32) for mu in (-2.0, 1.5, 4.0)]
    rule = TM.rule(adapt=0.3)
    r = renderer_mod.Renderer(W, H)
    prev = wprev = 0.0
    seen = []
    for k, img in enumerate(images):
        got = r.tonemap(img, prev_exposure=prev, rule=r.tonemap_rule(**rule), want_hist=True)
        c, A = TM.from_image(img)
        want = TM.tonemap(c, A, rule, T, W, H, prev=wprev)
        _same(got, want, k)
        prev, wprev = got[1], want[1]
        seen.append(float(want[1]))
    targets = [float(TM.exposure(TM.histogram(*TM.from_image(img)), rule)) for img in images]
    assert seen[0] == targets[0] and targets[1] < seen[1] < seen[0] and targets[2] < seen[2] < seen[1]      # the first is undamped, the others lag
    r.close()


# ---------------------------------------------------------------------------------------------------------------- the PNG

def _decode_png(data):
    """(W, H, the RGB bytes) of an 8-bit RGB PNG whose scanlines use filter 0: signature, IHDR, IDAT and IEND with their CRCs"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body)
        chunks.append((kind, body))
        at += 12 + n
    assert [k for k, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT")), np.uint8).reshape(h, 3 * w + 1)
    assert (raw[:, 0] == 0).all()
    return w, h, raw[:, 1:].reshape(h, w, 3)


def test_the_png_decodes_to_the_bytes_of_pt_tonemap(pt, renderer_mod, tmp_path):
    img = _special_image(48, 27, seed=5)
    for kw in (dict(), dict(devices=[0, 0])):
        r = _rendered(pt, renderer_mod, **kw)
        for k, image in enumerate((None, img)):
            path = tmp_path / f"tm_{k}.png"
            e = r.tonemap_png(path, image, prev_exposure=2.0, rule=r.tonemap_rule(adapt=0.5))
            rgb, e2 = r.tonemap(image, prev_exposure=2.0, rule=r.tonemap_rule(adapt=0.5))
            w, h, got = _decode_png(path.read_bytes())
            assert (w, h) == (48, 27) and np.array_equal(got, rgb) and e == e2 and rgb.max() > 0
        r.close()


# ---------------------------------------------------------------------------------------------------------------- refusals

def test_every_refusal_leaves_the_outputs_as_they_were(pt, renderer_mod, tmp_path):
    r = _rendered(pt, renderer_mod)
    L = r._L
    img = np.ones((27, 48, 4), f32)
    before = r.read_frame()

    def refused(rule, prev=0.0, image=None, code=-1):
        rgb, hist, e = np.full(48 * 27 * 3, 9, np.uint8), np.full(512, 5, np.uint32), C.c_float(7.0)
        rc = L.pt_tonemap(r._h, None if rule is None else C.byref(rule), None if image is None else image.ctypes.data, prev, rgb.ctypes.data, C.byref(e),
                          hist.ctypes.data)
        text = L.pt_last_error().decode()
        assert rc == code and text.startswith("pt_tonemap: "), (rc, text)
        assert (rgb == 9).all() and (hist == 5).all() and e.value == 7.0, text
        rc = L.pt_tonemap_save_png(r._h, None if rule is None else C.byref(rule), None if image is None else image.ctypes.data, prev,
                                   str(tmp_path / "never.png").encode(), C.byref(e))
        assert rc == code and L.pt_last_error().decode().startswith("pt_tonemap_save_png: ") and e.value == 7.0
        assert not (tmp_path / "never.png").exists()
        return text

    assert "null rule" in refused(None)
    bad = dict(curve=(-1, 3), transfer=(-1, 2), exposure=(-1.0, INF, NAN), key=(0.0, -1.0, INF, NAN), lo_pct=(-0.1, 1.0, NAN), hi_pct=(0.10, 0.05, 1.5, NAN),
               min_exposure=(0.0, -1.0, INF, NAN), max_exposure=(2.0 ** -11, INF, NAN), white=(0.0, -4.0, INF, NAN), adapt=(0.0, -0.5, 1.5, NAN))
    for name, values in bad.items():
        for v in values:
            for image in (None, img):
                assert "rule." + name in refused(r.tonemap_rule(**{name: v}), image=image), (name, v)
    for prev in (-1.0, -DENORM, INF, -INF, NAN):
        assert "prev_exposure" in refused(r.tonemap_rule(), prev=prev)
    assert "rule.curve" in refused(r.tonemap_rule(curve=7, adapt=0.0), prev=-1.0)        # the struct's order, prev_exposure last
    # the PNG's own: a null path, a file that cannot be written
    e = C.c_float(7.0)
    rule = r.tonemap_rule()
    assert L.pt_tonemap_save_png(r._h, C.byref(rule), None, 0.0, None, C.byref(e)) == -1 and L.pt_last_error() == b"pt_tonemap_save_png: null argument"
    nowhere = str(tmp_path / "no_such_directory" / "x.png").encode()
    assert L.pt_tonemap_save_png(r._h, C.byref(rule), None, 0.0, nowhere, C.byref(e)) == -1
    assert L.pt_last_error() == b"pt_tonemap_save_png: cannot open " + nowhere and e.value == 7.0
    # a null context, with a device in the process
    assert L.pt_tonemap(None, C.byref(rule), None, 0.0, None, C.byref(e), None) == -1 and e.value == 7.0
    # every output is optional, and the calls still go through
    assert L.pt_tonemap(r._h, C.byref(rule), None, 0.0, None, None, None) == 0
    assert L.pt_tonemap(r._h, C.byref(rule), None, 0.0, None, C.byref(e), None) == 0 and e.value == r.tonemap()[1] != 7.0
    assert frames_equal(r.read_frame(), before)
    r.close()
