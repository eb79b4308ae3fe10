"""GPU: adaptive sampling (include/pt_adaptive.h) against a float32 model fed with the oracle's per-frame images.

Every pixel-frame the adaptive stream traces is the reference's own job, so the oracle's one-frame image of frame f (frame count 1
overwrites FRAME) is exactly the `col` that frame adds to each pixel.  The model replays the statistics, the selection and the FRAME
accumulation; the GPU image must equal it bit for bit (NaN == NaN)."""
import numpy as np
import pytest

from _adaptive_model import Model
from conftest import frames_equal
from test_gpu_parity import _no_vn_workload

pytestmark = pytest.mark.gpu

W, H = 128, 72
NF = 16                                   # frames the oracle renders per scene


def _seeds(pt, first, n):
    return [pt.scenes.frame_seed(f) for f in range(first, first + n)]


def _cols(pt, oracle, wl):
    sc = oracle.Scene.from_workload(wl)
    return [oracle.render(sc, W, H, 1, pt.scenes.frame_seed(f), nthreads=8)[0][..., :3].copy() for f in range(1, NF + 1)]


@pytest.fixture(scope="module")
def c3(pt, oracle):
    wl = pt.scenes.build("C3", W, H)
    return wl, _cols(pt, oracle, wl)


@pytest.fixture(scope="module")
def novn(pt, oracle):
    wl = _no_vn_workload(pt, W, H)
    return wl, _cols(pt, oracle, wl)


def _open(renderer_mod, wl, **kw):
    r = renderer_mod.Renderer(W, H, **kw)
    r.load_workload(wl)
    r.reset_frame()
    return r


# (first_frame, n_frames, rel_err, abs_err, min_frames, max_frames) of successive adaptive calls
CALLS = [(1, 2, 0.05, 0.0, 2, 0), (3, 2, 0.05, 0.0, 2, 0), (5, 3, 0.05, 0.002, 4, 0), (8, 2, 0.02, 0.0, 4, 9), (10, 2, 0.05, 0.0, 4, 0)]
# the no-vn scene is nearly noise-free outside its NaN pixels: only a tight tolerance leaves a few pixels active (chosen with the oracle)
NOVN_CALLS = [(1, 2, 0.001, 0.0, 2, 0), (3, 2, 0.001, 0.0, 2, 0), (5, 2, 0.001, 0.0, 4, 0), (7, 2, 0.001, 0.0, 4, 0)]


def _run_exact(pt, renderer_mod, wl, cols, calls=CALLS, **kw):
    r = _open(renderer_mod, wl, **kw)
    m = Model(cols)
    counts, partial = [], False
    for first, n, rel, ab, mn, mx in calls:
        before = r.read_frame()[..., 3].copy()
        got_n = r.render_adaptive(first, _seeds(pt, first, n), rel, ab, mn, mx)
        act = m.adaptive(first, n, rel, ab, mn, mx)
        got = r.read_frame()
        assert frames_equal(got, m.F), f"call at frame {first}: {int((~((got == m.F) | (np.isnan(got) & np.isnan(m.F)))).sum())} floats differ"
        assert np.array_equal(got[..., 3] > before, act)
        assert got_n == int(act.sum())
        counts.append(got_n)
        partial = partial or 0 < got_n < W * H
    r.close()
    assert partial, counts                     # the parameters must exercise a real subsequence
    return counts, m.F


def test_exact_model_c3(pt, renderer_mod, c3):
    _run_exact(pt, renderer_mod, *c3)


def test_exact_model_no_vn_nan_pixels(pt, renderer_mod, novn):
    wl, cols = novn
    counts, F = _run_exact(pt, renderer_mod, wl, cols, NOVN_CALLS)
    assert np.isnan(F[..., :3]).any(axis=2).any()             # NaN pixels present; the model above stops them (every comparison false)


def test_sharding_invariance(pt, renderer_mod, c3):
    wl, cols = c3
    counts1, F1 = _run_exact(pt, renderer_mod, wl, cols)
    counts2, F2 = _run_exact(pt, renderer_mod, wl, cols, devices=[0, 0])
    assert counts1 == counts2 and frames_equal(F1, F2)
    # one shard of two behind pt_create: its own pixels, its own count
    m = Model(cols)
    own = np.zeros(W * H, bool)
    own[renderer_mod.shard_map(W, H, 1, 2)[renderer_mod.shard_map(W, H, 1, 2) >= 0]] = True
    own = own.reshape(H, W)
    r = _open(renderer_mod, wl, shard_rank=1, shard_count=2)
    for first, n, rel, ab, mn, mx in CALLS[:3]:
        got_n = r.render_adaptive(first, _seeds(pt, first, n), rel, ab, mn, mx)
        act = m.adaptive(first, n, rel, ab, mn, mx)
        assert got_n == int((act & own).sum())
    got = r.read_frame()
    r.close()
    assert frames_equal(got[own], m.F[own])


def test_all_active_equals_uniform(pt, renderer_mod, c3):
    wl, _ = c3
    r = _open(renderer_mod, wl)
    assert r.render_adaptive(1, _seeds(pt, 1, 3), 0.05, min_frames=100) == W * H
    assert r.render_adaptive(4, _seeds(pt, 4, 3), 0.05, min_frames=100) == W * H
    a = r.read_frame()
    r.reset_frame()
    r.render_batch(1, _seeds(pt, 1, 6))
    b = r.read_frame()
    r.close()
    assert frames_equal(a, b)


def test_stream_hand_off(pt, renderer_mod, c3):
    wl, cols = c3
    # adaptive calls, then ordinary batches: they render every pixel again (no stale active list)
    r = _open(renderer_mod, wl)
    m = Model(cols)
    for first, n, rel, ab, mn, mx in CALLS[:3]:
        r.render_adaptive(first, _seeds(pt, first, n), rel, ab, mn, mx)
        m.adaptive(first, n, rel, ab, mn, mx)
    r.render_batch(8, _seeds(pt, 8, 2))
    m.uniform(8, 2)
    assert frames_equal(r.read_frame(), m.F)
    r.render_batch_async(10, _seeds(pt, 10, 2))
    m.uniform(10, 2)
    assert frames_equal(r.read_frame(), m.F)
    r.close()
    # asynchronous batches in flight before an adaptive call land in FRAME but not in the statistics
    r = _open(renderer_mod, wl)
    m = Model(cols)
    r.render_batch_async(1, _seeds(pt, 1, 2))
    r.render_batch_async(3, _seeds(pt, 3, 2))
    m.uniform(1, 4)
    assert r.render_adaptive(5, _seeds(pt, 5, 2), 0.05, min_frames=2) == W * H       # T still zero: every pixel below min_frames
    m.adaptive(5, 2, 0.05, 0.0, 2, 0)
    n = r.render_adaptive(7, _seeds(pt, 7, 2), 0.05, min_frames=2)
    act = m.adaptive(7, 2, 0.05, 0.0, 2, 0)
    assert n == int(act.sum()) and frames_equal(r.read_frame(), m.F)
    # pt_reset_frame, pt_write_frame and pt_next_image zero the statistics
    saved = r.read_frame()
    assert r.render_adaptive(9, _seeds(pt, 9, 1), 0.05, min_frames=2) < W * H
    r.reset_frame()
    assert r.render_adaptive(1, _seeds(pt, 1, 2), 0.05, min_frames=2) == W * H
    r.write_frame(saved)
    assert r.render_adaptive(9, _seeds(pt, 9, 1), 0.05, min_frames=2) == W * H
    r.next_image()
    assert r.render_adaptive(1, _seeds(pt, 1, 2), 0.05, min_frames=2) == W * H
    r.close()


def _display_mean_model(F, java_bytes):
    with np.errstate(all="ignore"):
        v = F[..., :3] / F[..., 3:4]
    t = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(1))).astype(np.float32)
    q = np.floor(t * np.float32(255.0) + np.float32(0.5)).astype(np.int64)
    if java_bytes:
        s = np.where(q >= 128, q - 256, q)
        pix = s[..., 0] * 65536 + s[..., 1] * 256 + s[..., 2]
        q = np.stack([(pix >> 16) & 0xff, (pix >> 8) & 0xff, pix & 0xff], axis=-1)
    return q.astype(np.uint8)[::-1]


def test_display_mean(pt, renderer_mod, c3):
    wl, cols = c3
    r = _open(renderer_mod, wl)
    r.render_batch(1, _seeds(pt, 1, 3))
    for jb in (True, False):
        assert np.array_equal(r.read_display_mean(jb), r.read_display(3, jb))
    r.reset_frame()
    m = Model(cols)
    for first, n, rel, ab, mn, mx in CALLS[:3]:
        r.render_adaptive(first, _seeds(pt, first, n), rel, ab, mn, mx)
        m.adaptive(first, n, rel, ab, mn, mx)
    F = r.read_frame()
    assert frames_equal(F, m.F) and len(np.unique(F[..., 3])) > 1
    for jb in (True, False):
        assert np.array_equal(r.read_display_mean(jb), _display_mean_model(F, jb))
    r.close()


def test_errors(pt, renderer_mod, c3):
    wl, _ = c3
    r = _open(renderer_mod, wl)
    s = _seeds(pt, 1, 2)
    for kw in (dict(min_frames=1), dict(max_frames=-1), dict(abs_err=-1.0), dict(abs_err=float("nan"))):
        with pytest.raises(renderer_mod.PtError) as e:
            r.render_adaptive(1, s, 0.05, **kw)
        assert e.value.code == -1, kw
    for rel in (-0.1, float("nan")):
        with pytest.raises(renderer_mod.PtError) as e:
            r.render_adaptive(1, s, rel)
        assert e.value.code == -1
    with pytest.raises(renderer_mod.PtError) as e:
        r.render_adaptive(1, [], 0.05)
    assert e.value.code == -1
    p = np.array(wl.buffers[4], np.float32).copy()
    p[10] = 1.0                                        # Parameters.DEBUG
    r.set_buffer(4, p)
    with pytest.raises(renderer_mod.PtError) as e:
        r.render_adaptive(1, s, 0.05)
    assert e.value.code == -5
    r.close()
    g = renderer_mod.Renderer(W, H, devices=[0, 0])
    g.load_workload(wl); g.set_buffer(4, p)
    with pytest.raises(renderer_mod.PtError) as e:
        g.render_adaptive(1, s, 0.05)
    assert e.value.code == -5
    g.close()
