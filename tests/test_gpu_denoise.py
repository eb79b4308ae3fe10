"""GPU: the a-trous denoiser (pt_denoise, pt_read_display_denoised; include/pt_denoise.h) against the float32 model of tests/_denoise_model.py,
on the feature records of real scenes and FRAMEs injected through pt_write_frame; its flags, errors, contexts and its effect on noise."""
import ctypes as C

import numpy as np
import pytest

from _denoise_model import denoise as model

pytestmark = pytest.mark.gpu

W, H = 96, 54
SIG = (0.5, 0.3, 0.05, 0.1)
INF = float("inf")


def _ctx(pt, renderer_mod, name="C3", **kw):
    wl = pt.scenes.build(name, W, H)
    r = renderer_mod.Renderer(W, H, **kw)
    r.load_workload(wl)
    return r, wl


def _frames(feat):
    """injected FRAMEs: random means and counts; two colours split along the hit codes (object edges); and the random one with NaN,
    infinite and never-rendered (alpha 0) pixels"""
    rs = np.random.RandomState(5)
    cnt = rs.randint(1, 9, size=(H, W, 1)).astype(np.float32)
    rnd = np.concatenate([rs.rand(H, W, 3).astype(np.float32) * cnt, cnt], -1)
    code = np.ascontiguousarray(feat[..., 7]).view(np.int32)
    two = np.zeros((H, W, 4), np.float32)
    two[..., 3] = 4.0
    two[..., :3] = np.where(((code & 1) == 1)[..., None], np.float32(3.6), np.float32(0.4))
    bad = rnd.copy()
    bad[3, 4, 0] = np.nan
    bad[10, 20, :3] = np.inf
    bad[20:23, 30:33] = (5.0, 6.0, 7.0, 0.0)
    return {"random": rnd, "two_colour": two, "nan_alpha0": bad}


@pytest.mark.parametrize("scene", ["C3", "T1", "C6"])
def test_gpu_matches_the_model(pt, renderer_mod, scene):
    r, _ = _ctx(pt, renderer_mod, scene)
    feat = r.read_features()
    cases = [(5, SIG), (3, (0.2, 0.1, 0.02, 0.05)), (2, (INF, INF, INF, INF)), (0, SIG), (8, (1.0, INF, 0.1, INF))]
    for fname, fr in _frames(feat).items():
        r.write_frame(fr)
        for it, sig in cases:
            got = r.denoise(it, *sig)
            want = model(fr, feat, it, *sig)
            assert np.allclose(got, want, rtol=1e-4, atol=1e-6, equal_nan=True), (scene, fname, it, sig, np.nanmax(np.abs(got - want)))
            assert np.array_equal(got[..., 3], fr[..., 3])
    r.close()


def test_denoise_leaves_frame_and_later_renders_alone(pt, renderer_mod):
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 7)]
    imgs = []
    for probe in (False, True):
        r, _ = _ctx(pt, renderer_mod)
        r.render_batch(1, seeds[:3])
        if probe:
            before = r.read_frame()
            r.denoise()
            r.read_display_denoised()
            assert np.array_equal(r.read_frame().view(np.uint32), before.view(np.uint32))
        r.render_batch(4, seeds[3:])
        imgs.append(r.read_frame())
        r.close()
    assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32))


@pytest.mark.parametrize("java_bytes", [True, False])
def test_display_is_the_display_conversion_of_the_denoised_mean(pt, oracle, renderer_mod, java_bytes):
    r, _ = _ctx(pt, renderer_mod)
    r.render_batch(1, [pt.scenes.frame_seed(f) for f in range(1, 4)])
    dn = r.denoise(4)
    disp = r.read_display_denoised(4, java_bytes=java_bytes)
    r.close()
    assert np.array_equal(disp, oracle.display(dn, 1, java_bytes))


def test_errors_and_unsupported_contexts(pt, renderer_mod):
    from pathtracer_0_amd.renderer import PtError
    r, _ = _ctx(pt, renderer_mod)
    for it, sig in ((-1, SIG), (9, SIG), (2, (0.0, 0.3, 0.05, 0.1)), (2, (0.5, -1.0, 0.05, 0.1)), (2, (0.5, 0.3, float("nan"), 0.1))):
        with pytest.raises(PtError) as e:
            r.denoise(it, *sig)
        assert e.value.code == -1, (it, sig)                        # PT_ERR_ARG
        with pytest.raises(PtError):
            r.read_display_denoised(it, *sig)
    L = r._L
    assert L.pt_denoise(r._h, 1, 0.5, 0.3, 0.05, 0.1, None) == -1
    assert L.pt_read_features(r._h, None) == -1
    assert L.pt_read_display_denoised(r._h, 1, 0.5, 0.3, 0.05, 0.1, 1, None) == -1
    assert L.pt_denoise(None, 1, 0.5, 0.3, 0.05, 0.1, C.c_void_p(1)) == -1
    r.close()
    for kw in (dict(shard_rank=0, shard_count=2), dict(devices=[0], first_shard=0, total_shards=2)):
        p, _ = _ctx(pt, renderer_mod, **kw)
        assert p.read_features().shape == (H, W, 16)              # features work on every context
        with pytest.raises(PtError) as e:
            p.denoise()
        assert e.value.code == -5                                   # PT_ERR_UNSUPPORTED
        with pytest.raises(PtError):
            p.read_display_denoised()
        for show in (lambda: p.read_display(1), p.read_display_mean):
            with pytest.raises(PtError) as e:
                show()
            assert e.value.code == -1                               # PT_ERR_ARG
        p.close()


def test_multi_stream_denoise_equals_single(pt, renderer_mod):
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 4)]
    out = []
    for kw in ({}, {"devices": [0, 0]}):
        r, _ = _ctx(pt, renderer_mod, **kw)
        r.render_batch(1, seeds)
        out.append((r.read_frame(), r.denoise(5)))
        r.close()
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))


def test_denoising_reduces_the_error_at_four_frames(pt, renderer_mod):
    r, _ = _ctx(pt, renderer_mod)
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 1025)]
    r.render_batch(1, seeds[:4])
    noisy = r.read_frame()
    dn = r.denoise()
    r.render_batch(5, seeds[4:])
    ref = r.read_frame()
    r.close()
    mean = lambda f: f[..., :3].astype(np.float64) / f[..., 3:4]           # noqa: E731
    e_noisy = np.sqrt(((mean(noisy) - mean(ref)) ** 2).mean())
    e_dn = np.sqrt(((dn[..., :3].astype(np.float64) - mean(ref)) ** 2).mean())
    assert e_dn < e_noisy, (e_dn, e_noisy)
