"""GPU: luminance moments for every render path and the variance-guided filter (include/pt_guided.h).

Moments: T after ordinary renders against a float32 replay of the oracle's one-frame images (frame count 1 overwrites FRAME, so the one-frame
image of a seed is exactly the `col` that frame adds), bit for bit.  Filter: against the float32 model of tests/_guided_model.py on the feature
records of real scenes, with FRAME and T injected through pt_write_frame / pt_write_moments."""
import ctypes as C

import numpy as np
import pytest

from _guided_model import denoise_guided as model
from _guided_model import lum
from _reproject_model import frame_in, overlay
from conftest import frames_equal

pytestmark = pytest.mark.gpu

W, H = 96, 54
NF = 6
INF = float("inf")
SIG = (4.0, 0.3, 0.05, 0.1)


def _seeds(pt, idx):
    return [pt.scenes.frame_seed(f) for f in idx]


@pytest.fixture(scope="module")
def c3(pt, oracle):
    wl = pt.scenes.build("C3", W, H)
    sc = oracle.Scene.from_workload(wl)
    cols = [oracle.render(sc, W, H, 1, pt.scenes.frame_seed(f), nthreads=8)[0][..., :3].copy() for f in range(1, NF + 1)]
    return wl, cols


def _open(renderer_mod, wl, **kw):
    r = renderer_mod.Renderer(W, H, **kw)
    r.load_workload(wl)
    r.reset_frame()
    return r


class Replay:
    """FRAME and T as k_accumulate_moments updates them: cols[k - 1] = the rgb of seed k"""

    def __init__(self, cols, skip=None):
        self.cols, self.skip = cols, skip
        self.F = np.zeros((H, W, 4), np.float32)
        self.T = np.zeros((H, W, 4), np.float32)

    def batch(self, first, seed_idx):
        m = np.ones((H, W), bool) if self.skip is None else ~self.skip
        for j, k in enumerate(seed_idx):
            c = self.cols[k - 1][m]
            Y = lum(c)
            if first + j == 1:
                self.F[m] = np.concatenate([c, np.ones((c.shape[0], 1), np.float32)], axis=1)
                self.T[m] = np.stack([Y, Y * Y, np.ones_like(Y), np.zeros_like(Y)], axis=1)
            else:
                self.F[m, :3] = self.F[m, :3] + c
                self.F[m, 3] = self.F[m, 3] + np.float32(1)
                T = self.T[m]
                self.T[m] = np.stack([T[:, 0] + Y, T[:, 1] + Y * Y, T[:, 2] + np.float32(1), np.zeros_like(Y)], axis=1)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- moments

@pytest.mark.parametrize("form", ["sync", "async", "multi"])
def test_moments_equal_the_replay(pt, renderer_mod, c3, form):
    wl, cols = c3
    r = _open(renderer_mod, wl, **({"devices": [0, 0]} if form == "multi" else {}))
    r.record_moments(True)
    m = Replay(cols)

    def run(first, idx):
        if form == "async":
            r.render_batch_async(first, _seeds(pt, idx))
        else:
            r.render_batch(first, _seeds(pt, idx))
        m.batch(first, idx)

    run(1, [1, 2, 3])
    run(4, [4, 5])
    if form == "async":
        r.finish_image()
    assert _bits_equal(r.read_moments(), m.T) and frames_equal(r.read_frame(), m.F)
    assert np.array_equal(r.read_moments()[..., 2], r.read_frame()[..., 3])        # T.n == FRAME.a
    run(1, [5, 6])                                                                 # frame 1 restarts FRAME and T
    if form == "async":
        r.finish_image()
    assert _bits_equal(r.read_moments(), m.T) and frames_equal(r.read_frame(), m.F)
    r.close()


def test_moments_skip_the_mouse_overlay(pt, renderer_mod, c3):
    wl, cols = c3
    mouse = np.array([30.0, 17.0, 0.0], np.float32)
    ov = overlay(W, H, frame_in(wl.buffers[4], wl.buffers[0], wl.buffers[1], mouse))
    assert ov.any()
    r = _open(renderer_mod, wl)
    r.set_buffer(2, mouse)
    r.record_moments(True)
    m = Replay(cols, skip=ov)
    r.render_batch(1, _seeds(pt, [1, 2, 3]))
    m.batch(1, [1, 2, 3])
    r.render_batch(4, _seeds(pt, [4]))
    m.batch(4, [4])
    T = r.read_moments()
    r.close()
    assert _bits_equal(T, m.T)
    assert (T[ov] == 0).all()


def test_frame_is_unchanged_and_off_goes_back(pt, renderer_mod, c3):
    wl, _ = c3
    imgs = []
    for on in (False, True):
        r = _open(renderer_mod, wl)
        r.record_moments(on)
        r.render_batch(1, _seeds(pt, [1, 2, 3]))
        r.render_batch_async(4, _seeds(pt, [4, 5]))
        r.render(6, pt.scenes.frame_seed(6))
        imgs.append(r.read_frame())
        if on:
            T = r.read_moments()
            assert np.array_equal(T[..., 2], imgs[-1][..., 3])
            r.record_moments(False)                                # back to k_accumulate: FRAME grows, T stays
            r.render_batch(7, _seeds(pt, [1, 2]))
            assert _bits_equal(r.read_moments(), T)
            assert (r.read_frame()[..., 3] == imgs[-1][..., 3] + 2).all()
        else:
            assert not r.read_moments().any()                      # never recorded: zeros
        r.close()
    assert _bits_equal(imgs[0], imgs[1])


@pytest.mark.parametrize("kw", [{}, {"devices": [0, 0]}])
def test_read_write_moments_round_trip(pt, renderer_mod, c3, kw):
    wl, _ = c3
    r = _open(renderer_mod, wl, **kw)
    r.record_moments(True)
    r.render_batch(1, _seeds(pt, [1, 2, 3]))
    F, T = r.read_frame(), r.read_moments()
    assert T[..., 2].max() == 3.0
    r.write_frame(F)                                               # zeroes T
    assert not r.read_moments().any()
    r.write_moments(T)
    assert _bits_equal(r.read_moments(), T) and _bits_equal(r.read_frame(), F)
    rs = np.random.RandomState(4)
    T2 = rs.rand(H, W, 4).astype(np.float32)
    r.write_moments(T2)
    assert _bits_equal(r.read_moments(), T2)
    r.close()
    # a context that never recorded: write_moments allocates T
    r = _open(renderer_mod, wl, **kw)
    r.write_moments(T2)
    assert _bits_equal(r.read_moments(), T2)
    r.close()


# ---------------------------------------------------------------------------------------------------------------- filter

def _inject(feat):
    """FRAME: random means and counts with NaN, infinite and never-rendered pixels; T: random moments, n independent of FRAME.a, many pixels
    below min_frames, a few NaN sums"""
    rs = np.random.RandomState(7)
    cnt = rs.randint(1, 9, size=(H, W, 1)).astype(np.float32)
    fr = np.concatenate([rs.rand(H, W, 3).astype(np.float32) * cnt, cnt], -1)
    fr[3, 4, 0] = np.nan
    fr[10, 20, :3] = np.inf
    fr[20:23, 30:33] = (5.0, 6.0, 7.0, 0.0)
    n = rs.randint(0, 9, size=(H, W)).astype(np.float32)
    Y = rs.rand(H, W).astype(np.float32)
    sY = (n * Y).astype(np.float32)
    sYY = (n * Y * Y * (1.0 + rs.rand(H, W) * 0.5)).astype(np.float32)
    T = np.stack([sY, sYY, n, np.zeros_like(n)], -1).astype(np.float32)
    T[40, 50, :2] = np.nan
    return fr, T


CASES = [(5, SIG, 4), (3, (1.0, INF, 0.1, INF), 2), (2, (INF, 0.3, 0.05, 0.1), 4), (0, SIG, 4), (8, (10.0, 0.2, 0.02, 0.05), 6)]


@pytest.mark.parametrize("scene", ["C3", "T1", "C6"])
def test_gpu_matches_the_model(pt, renderer_mod, scene):
    wl = pt.scenes.build(scene, W, H)
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl)
    feat = r.read_features()
    fr, T = _inject(feat)
    r.write_frame(fr)
    r.write_moments(T)
    for it, sig, mf in CASES:
        got = r.denoise_guided(it, *sig, min_frames=mf)
        want = model(fr, feat, T, it, *sig, mf)
        assert np.allclose(got, want, rtol=1e-4, atol=1e-6, equal_nan=True), (scene, it, sig, mf, np.nanmax(np.abs(got - want)))
        assert np.array_equal(got[..., 3], fr[..., 3])
    assert _bits_equal(r.read_frame(), fr) and _bits_equal(r.read_moments(), T)     # neither is modified
    r.close()


@pytest.mark.parametrize("java_bytes", [True, False])
def test_display_is_the_display_conversion(pt, oracle, renderer_mod, c3, java_bytes):
    wl, _ = c3
    r = _open(renderer_mod, wl)
    r.record_moments(True)
    r.render_batch(1, _seeds(pt, [1, 2, 3]))
    dn = r.denoise_guided(4)
    disp = r.read_display_denoised_guided(4, java_bytes=java_bytes)
    r.close()
    assert np.array_equal(disp, oracle.display(dn, 1, java_bytes))


def test_multi_stream_equals_single(pt, renderer_mod, c3):
    wl, _ = c3
    out = []
    for kw in ({}, {"devices": [0, 0]}):
        r = _open(renderer_mod, wl, **kw)
        r.record_moments(True)
        r.render_batch(1, _seeds(pt, [1, 2, 3]))
        out.append((r.read_frame(), r.read_moments(), r.denoise_guided(5)))
        r.close()
    for a, b in zip(*out):
        assert _bits_equal(a, b)


def test_errors_and_unsupported_contexts(pt, renderer_mod, c3):
    from pathtracer_0_amd.renderer import PtError
    wl, _ = c3
    r = _open(renderer_mod, wl)
    r.render_batch(1, _seeds(pt, [1, 2]))
    with pytest.raises(PtError) as e:                              # no moments
        r.denoise_guided()
    assert e.value.code == -1 and "pt_record_moments" in str(e.value)
    r.record_moments(True)
    r.render_batch(3, _seeds(pt, [3]))
    for it, sig, mf in ((-1, SIG, 4), (9, SIG, 4), (2, SIG, 1), (2, (0.0, 0.3, 0.05, 0.1), 4), (2, (4.0, -1.0, 0.05, 0.1), 4),
                        (2, (4.0, 0.3, float("nan"), 0.1), 4), (2, (float("nan"), 0.3, 0.05, 0.1), 4)):
        with pytest.raises(PtError) as e:
            r.denoise_guided(it, *sig, min_frames=mf)
        assert e.value.code == -1, (it, sig, mf)                    # PT_ERR_ARG
        with pytest.raises(PtError):
            r.read_display_denoised_guided(it, *sig, min_frames=mf)
    L = r._L
    assert L.pt_denoise_guided(r._h, 1, 4.0, 0.3, 0.05, 0.1, 4, None) == -1
    assert L.pt_read_display_denoised_guided(r._h, 1, 4.0, 0.3, 0.05, 0.1, 4, 1, None) == -1
    assert L.pt_denoise_guided(None, 1, 4.0, 0.3, 0.05, 0.1, 4, C.c_void_p(1)) == -1
    assert L.pt_read_moments(r._h, None) == -1 and L.pt_write_moments(r._h, None) == -1
    assert L.pt_record_moments(None, 1) == -1
    r.close()
    for kw in (dict(shard_rank=0, shard_count=2), dict(devices=[0], first_shard=0, total_shards=2)):
        p = _open(renderer_mod, wl, **kw)
        p.record_moments(True)                                      # recording works on every context
        p.render_batch(1, _seeds(pt, [1, 2]))
        for call in (p.denoise_guided, p.read_display_denoised_guided, p.read_moments, lambda: p.write_moments(np.zeros((H, W, 4), np.float32))):
            with pytest.raises(PtError) as e:
                call()
            assert e.value.code == -5                               # PT_ERR_UNSUPPORTED
        p.close()


def test_converged_pixels_pass_through(pt, renderer_mod, c3):
    """T = (0, 0, 8): v = 0 everywhere, so no tap of another luminance weighs anything"""
    wl, _ = c3
    r = _open(renderer_mod, wl)
    r.record_moments(True)
    r.render_batch(1, _seeds(pt, [1, 2, 3, 4]))
    fr = r.read_frame()
    T = np.zeros((H, W, 4), np.float32)
    T[..., 2] = 8.0
    r.write_moments(T)
    got = r.denoise_guided(5)
    r.close()
    mean = fr[..., :3] / fr[..., 3:4]
    ok = np.isfinite(mean).all(-1) & (fr[..., 3] > 0)
    assert np.allclose(got[..., :3][ok], mean[ok], rtol=1e-6, atol=1e-6)     # (w c) / w rounds: 1 ulp of the brightest pixels is 2e-6


def test_guided_reduces_the_error_at_four_frames(pt, renderer_mod, c3):
    wl, _ = c3
    r = _open(renderer_mod, wl)
    r.record_moments(True)
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 1025)]
    r.render_batch(1, seeds[:4])
    noisy = r.read_frame()
    dn = r.denoise_guided()
    r.record_moments(False)
    r.render_batch(5, seeds[4:])
    ref = r.read_frame()
    r.close()
    mean = lambda f: f[..., :3].astype(np.float64) / f[..., 3:4]           # noqa: E731
    e_noisy = np.sqrt(((mean(noisy) - mean(ref)) ** 2).mean())
    e_dn = np.sqrt(((dn[..., :3].astype(np.float64) - mean(ref)) ** 2).mean())
    assert e_dn < e_noisy, (e_dn, e_noisy)
