"""GPU: adaptive sampling (include/pt_adaptive.h) where the small images of tests/test_gpu_adaptive.py never go: 1080p, where the block
scan of k_adaptive_scan carries a running total across many chunks of 256 block counts; active counts chosen at the wave and block
boundaries of select, compact and k_accumulate_adaptive (1, 2, 63..65, 255..257, 65535..65537); and images of a few pixels.

The per-frame colours of the model come from the GPU's uniform path (pinned to the oracle bit for bit by tests/test_gpu_parity.py):
frame f rendered alone with frame number 1 and frame f's seed, so that it overwrites FRAME, then read back.  A lattice of every such
image is checked against the oracle here as well."""
import numpy as np
import pytest

from _adaptive_model import Model, rel_ratio, select, tolerance_for_count
from conftest import frames_equal

W, H = 1920, 1080
NF = 12
# (first_frame, n_frames, rel_err, abs_err, min_frames, max_frames) of successive adaptive calls at 1080p.  The first call renders every
# pixel (T is zero, so every n is below min_frames); each later one leaves 10 % .. 90 % of the pixels active.
CALLS = [(1, 2, 0.5, 0.0, 2, 0), (3, 2, 0.5, 0.0, 2, 0), (5, 3, 0.3, 0.002, 2, 0), (8, 2, 0.2, 0.0, 2, 12), (10, 3, 0.1, 0.0, 2, 0)]
KW, KH = 640, 512                          # the chosen-count image: 327680 pixels, 1280 blocks of 256
KS = [1, 2, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537]


def _seeds(pt, first, n):
    return [pt.scenes.frame_seed(f) for f in range(first, first + n)]


def _open(renderer_mod, wl, w, h, **kw):
    r = renderer_mod.Renderer(w, h, **kw)
    r.load_workload(wl)
    r.reset_frame()
    return r


def _gpu_cols(pt, renderer_mod, wl, w, h, nf):
    """cols[f - 1]: the rgb frame f adds to every pixel, from the uniform path (frame number 1 overwrites FRAME)"""
    r = _open(renderer_mod, wl, w, h)
    cols = []
    for f in range(1, nf + 1):
        r.reset_frame()
        r.render(1, pt.scenes.frame_seed(f))
        cols.append(r.read_frame()[..., :3].copy())
    r.close()
    return cols


def _differ(a, b):
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


def test_frame_number_only_selects_the_overwrite(pt, oracle):
    """on the oracle: frame f rendered onto a zeroed FRAME with its own frame number gives the colour that frame number 1 gives"""
    w, h = 96, 54
    sc = oracle.Scene.from_workload(pt.scenes.build("C3", w, h))
    for f in (2, 3, 7, 12, 1000):
        one = oracle.render(sc, w, h, 1, pt.scenes.frame_seed(f), nthreads=8)[0]
        own = oracle.render(sc, w, h, f, pt.scenes.frame_seed(f), nthreads=8)[0]
        assert frames_equal(one, own), f


@pytest.fixture(scope="module")
def full(pt, oracle, renderer_mod):
    wl = pt.scenes.build("C3", W, H)
    cols = _gpu_cols(pt, renderer_mod, wl, W, H, NF)
    sc = oracle.Scene.from_workload(wl)
    for f in range(1, NF + 1):                                 # every image against the oracle on a lattice of 80 x 40 pixels
        o = oracle.render(sc, W, H, 1, pt.scenes.frame_seed(f), nthreads=8, xs=24, ys=27)[0]
        assert frames_equal(cols[f - 1][::27, ::24], o[::27, ::24, :3]), f"frame {f}: {_differ(cols[f - 1][::27, ::24], o[::27, ::24, :3])} floats differ"
    return wl, cols


def _run_full(pt, renderer_mod, wl, cols, **kw):
    r = _open(renderer_mod, wl, W, H, **kw)
    m = Model(cols)
    counts = []
    for i, (first, n, rel, ab, mn, mx) in enumerate(CALLS):
        got_n = r.render_adaptive(first, _seeds(pt, first, n), rel, ab, mn, mx)
        act = m.adaptive(first, n, rel, ab, mn, mx)
        got = r.read_frame()
        assert frames_equal(got, m.F), f"call at frame {first}: {_differ(got, m.F)} floats differ"
        assert got_n == int(act.sum()), (first, got_n, int(act.sum()))
        assert (i == 0 and got_n == W * H) or 0.1 * W * H <= got_n <= 0.9 * W * H, (first, got_n)
        counts.append(got_n)
    r.close()
    return counts, m.F


@pytest.mark.gpu
def test_full_size_one_and_two_streams(pt, renderer_mod, full):
    wl, cols = full
    c1, F1 = _run_full(pt, renderer_mod, wl, cols)
    c2, F2 = _run_full(pt, renderer_mod, wl, cols, devices=[0, 0])
    assert c1 == c2 and frames_equal(F1, F2)


@pytest.mark.gpu
def test_full_size_one_shard_of_two(pt, renderer_mod, full):
    wl, cols = full
    sm = renderer_mod.shard_map(W, H, 1, 2)
    own = np.zeros(W * H, bool)
    own[sm[sm >= 0]] = True
    own = own.reshape(H, W)
    r = _open(renderer_mod, wl, W, H, shard_rank=1, shard_count=2)
    m = Model(cols)
    for first, n, rel, ab, mn, mx in CALLS:
        got_n = r.render_adaptive(first, _seeds(pt, first, n), rel, ab, mn, mx)
        act = m.adaptive(first, n, rel, ab, mn, mx)
        assert got_n == int((act & own).sum()), (first, got_n, int((act & own).sum()))
        got = r.read_frame()
        assert frames_equal(got[own], m.F[own]), f"call at frame {first}: {_differ(got[own], m.F[own])} floats differ"
    r.close()


@pytest.fixture(scope="module")
def counts_img(pt, renderer_mod):
    wl = pt.scenes.build("C3", KW, KH)
    cols = _gpu_cols(pt, renderer_mod, wl, KW, KH, 7)
    base = Model(cols)
    base.adaptive(1, 4, 0.0, 0.0, 100)                          # every pixel 4 frames
    return wl, cols, base


def _chosen(pt, renderer_mod, counts_img, ks, **kw):
    wl, cols, base = counts_img
    r = _open(renderer_mod, wl, KW, KH, **kw)
    for k in ks:
        tol = tolerance_for_count(base.T, k, 4)
        assert tol is not None, k
        rel, ab = tol
        assert int(select(base.T, rel, ab, 4, 0).sum()) == k
        for n in (1, 3):
            r.reset_frame()
            assert r.render_adaptive(1, _seeds(pt, 1, 4), 0.0, 0.0, 100) == KW * KH
            m = Model(cols)
            m.F, m.T = base.F.copy(), base.T.copy()
            got_n = r.render_adaptive(5, _seeds(pt, 5, n), rel, ab, 4, 0)
            act = m.adaptive(5, n, rel, ab, 4, 0)
            got = r.read_frame()
            assert got_n == k == int(act.sum()), (k, n, got_n)
            assert frames_equal(got, m.F), f"k={k} n={n}: {_differ(got, m.F)} floats differ"
    r.close()


@pytest.mark.gpu
def test_chosen_active_counts(pt, renderer_mod, counts_img):
    # the relative ranking cannot reach these counts on C3 (most noisy pixels have one non-black frame of four: ratio 1), so at least
    # the large counts take the abs_err ranking; the assert keeps the count reachable as the scene changes
    assert np.isfinite(rel_ratio(counts_img[2].T)[1]).sum() > max(KS)
    _chosen(pt, renderer_mod, counts_img, KS)


@pytest.mark.gpu
def test_chosen_active_counts_two_streams(pt, renderer_mod, counts_img):
    _chosen(pt, renderer_mod, counts_img, [1, 257], devices=[0, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (1, 37), (8, 8), (13, 5), (16, 16)])
def test_tiny_images_all_active_equal_uniform(pt, renderer_mod, w, h):
    wl = pt.scenes.build("C3", w, h)
    r = _open(renderer_mod, wl, w, h)
    assert r.render_adaptive(1, _seeds(pt, 1, 3), 0.05, min_frames=100) == w * h
    assert r.render_adaptive(4, _seeds(pt, 4, 1), 0.05, min_frames=100) == w * h
    assert r.render_adaptive(5, _seeds(pt, 5, 2), 0.05, min_frames=100) == w * h
    a = r.read_frame()
    r.reset_frame()
    r.render_batch(1, _seeds(pt, 1, 6))
    b = r.read_frame()
    r.close()
    assert frames_equal(a, b)
