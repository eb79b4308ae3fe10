"""GPU: first-hit feature records (pt_read_features, include/pt_denoise.h) against the oracle's rayScene, a float64 model of main()'s camera
ray, a bilinear-REPEAT model of map_Kd, pt_debug_intersect, and across context kinds."""
import numpy as np
import pytest

from _reproject_ref64 import camera_dirs as _camera_dirs
from test_gpu_parity import _no_vn_workload

pytestmark = pytest.mark.gpu

W, H = 48, 27
NPIX = 400                                          # pixels per scene checked against the oracle (a fixed random subset)


def _i32(a):
    return np.asarray(a, np.float32).view(np.int32)


def _feat(renderer_mod, wl, W=W, H=H, **ctx):
    r = renderer_mod.Renderer(W, H, **ctx)
    r.load_workload(wl)
    f = r.read_features()
    r.close()
    return f


def _mats(wl):
    m = np.asarray(wl.buffers[14], np.float32).reshape(-1)
    me = int(m[0])
    n = (m.size - 1) // me
    return [m[me * k: me * k + me] for k in range(n)]


def _workloads(pt):
    S = pt.scenes
    out = [(n, S.build(n, W if n != "C1" else 48, H if n != "C1" else 48)) for n in ("C1", "C2", "C3", "C4", "C5", "C6", "T1")]
    out.append(("no_vn", _no_vn_workload(pt, W, H)))
    c2 = S.build("C2", W, H)
    b = dict(c2.buffers); b[1] = np.array([0.15, -0.4, 0.3], np.float32)
    out.append(("C2_rotated", S.Workload("C2_rotated", W, H, b, c2.sky, c2.sample_res, c2.max_bounces, c2.info)))
    c3 = S.build("C3", W, H)
    out.append(("C3_blur_af0", c3.with_params(BLUR=0.05, AUTO_FOCUS=0, FOCAL_DISTANCE=2.5)))
    out.append(("C3_blur_af1", c3.with_params(BLUR=0.05, AUTO_FOCUS=1)))
    return out


@pytest.fixture(scope="module")
def scenes(pt):
    return _workloads(pt)


@pytest.mark.parametrize("k", range(11))
def test_features_match_the_oracle(pt, oracle, renderer_mod, scenes, k):
    name, wl = scenes[k]
    h, w = wl.H, wl.W
    f = _feat(renderer_mod, wl, w, h)
    mats = _mats(wl)
    sc = oracle.Scene.from_workload(wl)
    org = np.asarray(wl.buffers[0], np.float32)
    rs = np.random.RandomState(k)
    pix = rs.choice(w * h, size=min(NPIX, w * h), replace=False)
    flat = f.reshape(-1, 16)
    hits = 0
    for p in pix:
        rec = flat[p]
        code, out = oracle.ray_scene(sc, org, rec[8:11])
        code = int(code) if code >= 0 else -1
        assert _i32(rec[7]) == code, (name, p, _i32(rec[7]), code)
        assert _i32(rec[0]) == _i32(out[0]), (name, p, rec[0], out[0])
        mat = int(_i32(rec[11]))
        assert mat == int(out[7]), (name, p, mat, out[7])
        if code < 0:
            assert np.array_equal(rec[1:7], np.zeros(6, np.float32)) and np.array_equal(rec[12:16], np.zeros(4, np.float32))
            continue
        hits += 1
        if mats[mat][37] <= -1:                                   # no map_norm: the normal is rayScene's
            assert np.array_equal(rec[1:4], out[4:7], equal_nan=True), (name, p, rec[1:4], out[4:7])
        if all(mats[mat][j] <= -1 for j in (22, 23, 24, 32, 33, 35, 37, 39, 41)):
            assert np.array_equal(rec[4:7], mats[mat][4:7]), (name, p, rec[4:7], mats[mat][4:7])
    assert hits > 0, name
    # every pixel's direction is main()'s lens-centre ray
    assert np.abs(f[..., 8:11] - _camera_dirs(wl, w, h)).max() < 1e-6, name


def test_no_vn_normals_stay_nan(pt, renderer_mod):
    """triangles without vertex normals shade with NaN normals: the records keep them, and the denoiser passes such pixels through"""
    f = _feat(renderer_mod, _no_vn_workload(pt, W, H))
    hit = _i32(f[..., 7]) >= 0
    nan = np.isnan(f[..., 1:4]).any(-1)
    assert hit.any() and nan.any() and not nan[~hit].any()


def _bilinear_repeat(tex, u, v):
    h, w = tex.shape[:2]
    fu, fv = u * w - 0.5, v * h - 0.5
    i0, j0 = int(np.floor(fu)), int(np.floor(fv))
    a, b = fu - i0, fv - j0
    t = tex[..., :3].astype(np.float64) / 255.0
    i0m, i1m, j0m, j1m = i0 % w, (i0 + 1) % w, j0 % h, (j0 + 1) % h
    return (1 - a) * (1 - b) * t[j0m, i0m] + a * (1 - b) * t[j0m, i1m] + (1 - a) * b * t[j1m, i0m] + a * b * t[j1m, i1m]


def test_mapped_albedo_and_uv(pt, renderer_mod):
    wl = pt.scenes.build("T1", 96, 54)
    f = _feat(renderer_mod, wl, 96, 54).reshape(-1, 16)
    mats = _mats(wl)
    checked = 0
    for rec in f:
        if _i32(rec[7]) < 0:
            continue
        m = mats[int(_i32(rec[11]))]
        if m[23] <= -1:
            continue
        want = _bilinear_repeat(wl.textures[int(m[23])], float(rec[12]), float(rec[13])) * m[4:7].astype(np.float64)
        assert np.abs(rec[4:7] - want).max() < 1e-3, (rec, want)
        checked += 1
    assert checked > 50


def test_full_size_c3_equals_debug_intersect(pt, renderer_mod):
    wl = pt.scenes.build("C3", 1920, 1080)
    r = renderer_mod.Renderer(1920, 1080)
    r.load_workload(wl)
    f = r.read_features().reshape(-1, 16)
    o = np.broadcast_to(np.asarray(wl.buffers[0], np.float32), (f.shape[0], 3))
    tuv, prim = r.debug_intersect(o, f[:, 8:11])
    r.close()
    hit = _i32(f[:, 7]) >= 0
    code = np.where(prim & 0x40000000, 3 * 0x1000000 + (prim & 0xFFFFFF), 0x1000000 + prim)
    live = (prim != -1) & (tuv[:, 0] < 1e25)
    assert np.array_equal(hit, live)
    assert np.array_equal(_i32(f[hit, 7]), code[hit])
    assert np.array_equal(_i32(f[hit, 0]), _i32(tuv[hit, 0]))
    assert (f[~hit, 0] == -1).all()


@pytest.mark.parametrize("kind", ["sharded", "multi_stream", "virtual_multi"])
def test_every_context_gives_the_same_features(pt, renderer_mod, monkeypatch, kind):
    wl = pt.scenes.build("C3", 96, 54)
    ref = _feat(renderer_mod, wl, 96, 54)
    if kind == "sharded":
        got = _feat(renderer_mod, wl, 96, 54, shard_rank=1, shard_count=3)
    elif kind == "multi_stream":
        got = _feat(renderer_mod, wl, 96, 54, devices=[0, 0])
    else:
        monkeypatch.setenv("PT_MULTI_VIRTUAL_DEVICES", "2")
        got = _feat(renderer_mod, wl, 96, 54, devices=[0, 0])
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_camera_change_recomputes(pt, renderer_mod):
    wl = pt.scenes.build("C2", 96, 54)
    r = renderer_mod.Renderer(96, 54)
    r.load_workload(wl)
    a = r.read_features()
    assert np.array_equal(r.read_features().view(np.uint32), a.view(np.uint32))      # reused
    cam = np.asarray(wl.buffers[0], np.float32) + np.float32(0.2)
    r.set_buffer(0, cam)
    b = r.read_features()
    r.close()
    b2 = dict(wl.buffers); b2[0] = cam
    moved = pt.scenes.Workload("C2_moved", 96, 54, b2, wl.sky, wl.sample_res, wl.max_bounces, wl.info)
    fresh = _feat(renderer_mod, moved, 96, 54)
    assert not np.array_equal(a, b)
    assert np.array_equal(b.view(np.uint32), fresh.view(np.uint32))


def test_features_between_renders_leave_frame_bit_identical(pt, renderer_mod):
    wl = pt.scenes.build("C3", 96, 54)
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 5)]
    imgs = []
    for probe in (False, True):
        r = renderer_mod.Renderer(96, 54)
        r.load_workload(wl)
        r.render_batch(1, seeds[:2])
        if probe:
            r.read_features()
        r.render_batch_async(3, seeds[2:])
        if probe:
            r.read_features()
        imgs.append(r.read_frame())
        r.close()
    assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32))
