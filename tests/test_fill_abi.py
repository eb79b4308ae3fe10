"""CPU: interleaved rendering (include/pt_fill.h) — exported symbols, a strict-C99 client, hand cases of the float32 model
(tests/_fill_model.py) that tests/test_gpu_fill.py holds the device to, and the oracle experiment the surface rests on."""
import ctypes
import os
import subprocess

import numpy as np

from _demod_model import denoise_guided_demod
from _denoise_model import features
from _fill_model import denoise_guided_filled, fill_frame, lattice
from _guided_model import denoise_guided, lum
from test_adaptive_abi import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
f32 = np.float32
NAMES = ["pt_denoise_guided_filled", "pt_fill_frame", "pt_read_display_denoised_guided_filled", "pt_render_interleaved"]
SIG = (2.0, 0.3, 0.05)                                  # the defaults' sigma_lum, sigma_normal, sigma_depth
GEO = SIG[1:]
H, W, NFR = 27, 48, 8
GREY, BLUE = f32([0.9, 0.9, 0.9]), f32([0.157, 0.235, 0.784])
MISS = -1


def test_hip_library_exports_the_fill_symbols(pt):
    from pathtracer_0_amd import build
    lib = ctypes.CDLL(build.build_hip())
    assert _declared("pt_fill.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), n
    for other in ("pt_api.h", "pt_adaptive.h", "pt_denoise.h", "pt_reproject.h", "pt_guided.h", "pt_steer.h", "pt_demod.h"):
        assert not set(NAMES) & set(_declared(other)), other


def test_fill_header_compiles_as_c99(tmp_path):
    src = tmp_path / "client.c"
    src.write_text('#include "pt_api.h"\n#include "pt_fill.h"\n#include <stddef.h>\n'
                   "int main(void) {\n"
                   "    int (*i)(pt_ctx*, int, int, const int32_t*, int, int, int, int64_t*) = pt_render_interleaved;\n"
                   "    int (*f)(pt_ctx*, float, float, float, float, float*, int64_t*) = pt_fill_frame;\n"
                   "    int (*d)(pt_ctx*, int, float, float, float, float, int, float, float*) = pt_denoise_guided_filled;\n"
                   "    int (*v)(pt_ctx*, int, float, float, float, float, int, float, int, uint8_t*) = pt_read_display_denoised_guided_filled;\n"
                   "    return (i == NULL) + (f == NULL) + (d == NULL) + (v == NULL);\n}\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "client.o")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr


# ---------------------------------------------------------------------------------------------------------------- hand cases of the model

def _set_mat(feat, where, mat):
    m = np.ascontiguousarray(feat[..., 11]).view(np.int32).copy()
    m[where] = mat
    feat[..., 11] = m.view(f32)


def _set_miss(feat, where):
    code = np.ascontiguousarray(feat[..., 7]).view(np.int32).copy()
    code[where] = MISS
    feat[..., 7] = code.view(f32)
    feat[where + (0,)] = -1.0
    feat[where + (slice(1, 7),)] = 0.0
    _set_mat(feat, where, -1)


def _checker_feat():
    feat = features(H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    chk = ((yy // 4 + xx // 4) % 2).astype(bool)
    feat[..., 4:7] = np.where(chk[..., None], GREY, BLUE)
    return feat


def _samples(Kd, noise=0.25, seed=5):
    """FRAME and T of NFR frames of colour Kd * E_k, E_k = 0.6 + noise * N(0, 1) per pixel and frame"""
    rs = np.random.RandomState(seed)
    E = (0.6 + noise * rs.randn(NFR, H, W)).astype(f32)
    col = (Kd[None] * E[..., None]).astype(f32)
    Y = lum(col)
    frame = np.concatenate([col.sum(0), np.full((H, W, 1), NFR, f32)], -1).astype(f32)
    T = np.stack([Y.sum(0), (Y * Y).sum(0), np.full((H, W), NFR, f32), np.zeros((H, W), f32)], -1).astype(f32)
    return frame, T


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


def _row(values, count=8.0):
    """a 1 x n FRAME of the means `values` with `count` frames each; None makes a hole"""
    fr = np.zeros((1, len(values), 4), f32)
    for x, v in enumerate(values):
        if v is not None:
            fr[0, x] = (v * count, v * count, v * count, count)
    return fr


def test_an_image_without_holes_is_unchanged():
    feat = _checker_feat()
    frame, T = _samples(feat[..., 4:7])
    frame[3, 5, 3] = np.nan                             # a NaN count is no hole
    for floor in (0.0, 0.2):
        out, n, d = fill_frame(frame, feat, *GEO, 0.1, floor, detail=True)
        assert n == 0 and not d["hole"].any() and _bits_equal(out, frame)
    want = denoise_guided(frame, feat, T, 3, *SIG, 0.1, 4)
    assert np.array_equal(denoise_guided_filled(frame, feat, T, 3, *SIG, 0.1, 4), want, equal_nan=True)
    want = denoise_guided_demod(frame, feat, T, 3, *SIG, INF, 4, 0.2)
    assert np.array_equal(denoise_guided_filled(frame, feat, T, 3, *SIG, INF, 4, 0.2), want, equal_nan=True)


def test_equal_weight_sources_add_their_counts():
    """k sources of the same weight and count A: A' = k * A, the count of the pooled mean (every operation here is exact)"""
    out, n = fill_frame(_row([0.25, None, 0.75]), features(1, 3), *GEO, 0.1)
    assert n == 1 and np.array_equal(out[0, 1], f32([0.5 * 16, 0.5 * 16, 0.5 * 16, 16.0]))
    # the four edge neighbours of a 3 x 3 image's centre (its corners are other holes)
    fr = np.zeros((3, 3, 4), f32)
    for y, x, v in ((0, 1, 0.125), (1, 0, 0.25), (1, 2, 0.5), (2, 1, 0.125)):
        fr[y, x] = (v * 4, v * 4, v * 4, 4.0)
    out, n, d = fill_frame(fr, features(3, 3), *GEO, 0.1, detail=True)
    assert np.array_equal(out[1, 1], f32([0.25 * 16, 0.25 * 16, 0.25 * 16, 16.0]))
    assert d["hole"].sum() == 5 and n == 5              # the corners fill from the same four, at other weights
    # unequal counts: two sources of equal weight with 2 and 6 frames carry the variance of 1/4 (1/2 + 1/6) = 1/6: A' = 6
    fr = _row([0.25, None, 0.75])
    fr[0, 0] = (0.5, 0.5, 0.5, 2.0)
    fr[0, 2] = (4.5, 4.5, 4.5, 6.0)
    out, _ = fill_frame(fr, features(1, 3), *GEO, 0.1)
    assert np.allclose(out[0, 1], [3.0, 3.0, 3.0, 6.0], rtol=1e-6, atol=0)


def test_a_hole_at_a_material_edge_takes_its_own_side():
    feat = features(1, 5)
    _set_mat(feat, (slice(None), slice(3, 5)), 1)
    fr = _row([1.0, 1.0, None, 5.0, 5.0])
    out, n = fill_frame(fr, feat, INF, INF, INF)        # no edge term helps: the material alone keeps the sides apart
    assert n == 1 and np.array_equal(out[0, 2, :3] / out[0, 2, 3], f32([1.0, 1.0, 1.0]))
    _set_mat(feat, (slice(None), slice(2, 3)), 1)
    out, _ = fill_frame(fr, feat, INF, INF, INF)
    assert np.array_equal(out[0, 2, :3] / out[0, 2, 3], f32([5.0, 5.0, 5.0]))
    # ... and the same surface across a normal edge: the normal term does it
    feat = features(1, 5)
    feat[0, 3:, 1:4] = (1.0, 0.0, 0.0)
    out, _ = fill_frame(fr, feat, 0.1, INF, INF)
    assert np.allclose(out[0, 2, :3] / out[0, 2, 3], 1.0, rtol=1e-6, atol=0)


def test_a_hole_without_a_source_stays_and_the_filter_passes_it_through():
    feat = features(1, 5)
    _set_mat(feat, (slice(None), slice(2, 3)), 7)       # a material of its own
    fr = _row([1.0, 1.0, None, 5.0, 5.0])
    fr[0, 2, :3] = (0.3, 0.2, 0.1)                      # raw rgb under a zero count
    T = np.zeros((1, 5, 4), f32)
    T[..., 0], T[..., 1], T[..., 2] = 8.0, 9.0, 8.0
    T[0, 2] = 0.0
    for floor in (0.0, 0.2):
        out, n, d = fill_frame(fr, feat, *GEO, 0.1, floor, detail=True)
        assert n == 0 and d["hole"].sum() == 1 and _bits_equal(out, fr)
        dn = denoise_guided_filled(fr, feat, T, 3, *SIG, 0.1, 4, floor)
        assert np.array_equal(dn[0, 2], f32([0.3, 0.2, 0.1, 0.0]))
    # a pixel without finite features is no hole, whatever lies around it
    feat = features(1, 3)
    feat[0, 1, 2] = np.nan
    out, n, d = fill_frame(_row([0.25, None, 0.75]), feat, *GEO, 0.1, detail=True)
    assert n == 0 and not d["hole"].any()


def test_a_miss_hole_uses_miss_sources_only():
    feat = features(1, 5)
    _set_miss(feat, (slice(None), slice(2, 5)))
    fr = _row([1.0, 1.0, None, 5.0, 3.0])
    out, n = fill_frame(fr, feat, *GEO, 0.1, 0.2)
    # weights h(1) h(0) and h(2) h(0) = 4 : 1
    assert n == 1 and np.allclose(out[0, 2, :3] / out[0, 2, 3], (4 * 5.0 + 3.0) / 5, rtol=1e-6, atol=0)
    # and a hit hole between misses finds nothing
    feat = features(1, 3)
    _set_miss(feat, (slice(None), slice(0, 1)))
    _set_miss(feat, (slice(None), slice(2, 3)))
    out, n = fill_frame(_row([0.25, None, 0.75]), feat, *GEO, 0.1)
    assert n == 0


def test_the_output_alpha_marks_the_reconstructed_pixels():
    feat = _checker_feat()
    frame, T = _samples(feat[..., 4:7])
    on = lattice(H, W, 2, 1, 0)
    frame[~on] = 0.0
    T[~on] = 0.0
    for floor in (0.0, 0.2):
        out = denoise_guided_filled(frame, feat, T, 3, *SIG, INF, 4, floor)
        assert np.array_equal(out[..., 3], frame[..., 3]) and np.isfinite(out).all()
        assert (out[..., :3][~on] > 0).all()            # no hole stays black


def test_a_checker_albedo_over_constant_illumination_comes_back_on_a_lattice():
    """colour = checker albedo * 0.6 on the (0, 0) lattice of stride 2 and nothing elsewhere: with the albedo term off the demodulated fill gives
    every hole its own texel (the illumination is constant), the plain fill the average of the texels around it"""
    feat = _checker_feat()
    Kd = feat[..., 4:7]
    truth = (Kd * f32(0.6)).astype(f32)
    on = lattice(H, W, 2, 0, 0)
    frame = np.concatenate([truth * f32(NFR), np.full((H, W, 1), NFR, f32)], -1).astype(f32)
    frame[~on] = 0.0
    out, n, d = fill_frame(frame, feat, *GEO, INF, 0.01, detail=True)
    assert n == int((~on).sum()) and np.array_equal(d["filled"], ~on)
    mean = out[..., :3] / out[..., 3:4]
    assert np.abs(mean / truth - 1).max() <= 1e-6, float(np.abs(mean / truth - 1).max())
    assert _bits_equal(out[on], frame[on])
    plain, _ = fill_frame(frame, feat, *GEO, INF, 0.0)
    assert np.abs(plain[..., :3] / plain[..., 3:4] / truth - 1).max() > 0.01
    # the albedo term brings the plain fill back where a hole has a source of its own texel
    edged, _ = fill_frame(frame, feat, *GEO, 0.01, 0.0)
    assert np.abs(edged[..., :3] / edged[..., 3:4] / truth - 1).max() <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- the oracle experiment

def _cpu_features(oracle, wl):
    """the feature records of include/pt_denoise.h from the oracle's rayScene along a float64 model of main()'s lens-centre ray (the records
    tests/test_gpu_features.py holds pt_read_features to); for scenes without textures"""
    from _reproject_ref64 import camera_dirs as _camera_dirs
    from test_gpu_features import _mats
    h, w = wl.H, wl.W
    mats = _mats(wl)
    assert all(m[j] <= -1 for m in mats for j in (22, 23, 24, 32, 33, 35, 37, 39, 41))
    sc = oracle.Scene.from_workload(wl)
    org = np.asarray(wl.buffers[0], f32)
    dirs = _camera_dirs(wl, w, h).astype(f32)
    feat = np.zeros((h, w, 16), f32)
    code = np.full((h, w), MISS, np.int32)
    mat = np.full((h, w), -1, np.int32)
    for y in range(h):
        for x in range(w):
            c, out = oracle.ray_scene(sc, org, dirs[y, x])
            feat[y, x, 0] = out[0]
            if c >= 0:
                code[y, x], mat[y, x] = int(c), int(out[7])
                feat[y, x, 1:4] = out[4:7]
                feat[y, x, 4:7] = mats[int(out[7])][4:7]
    feat[..., 7] = code.view(f32)
    feat[..., 8:11] = dirs
    feat[..., 11] = mat.view(f32)
    return feat


def _accumulate(oracle, sc, w, h, seeds, **kw):
    """FRAME and T of the frames 1 .. len(seeds), as the render path and include/pt_guided.h accumulate them; kw: the oracle's pixel stride"""
    frame = np.zeros((h, w, 4), f32)
    T = np.zeros((h, w, 4), f32)
    threads = max(1, min(8, os.cpu_count() or 1))
    for k, seed in enumerate(seeds):
        one, _ = oracle.render(sc, w, h, k + 1, int(seed), None, threads, **kw)
        done = one[..., 3] > 0
        Y = lum(one[..., :3])
        frame[done] = (frame[done] + one[done]).astype(f32)
        T[done] = (T[done] + np.stack([Y, Y * Y, np.ones_like(Y), np.zeros_like(Y)], -1)[done]).astype(f32)
    return frame, T


def _clamped_rmse(img, ref):
    ok = np.isfinite(img).all(-1) & np.isfinite(ref).all(-1)
    d = np.clip(img[ok], 0, 1).astype(np.float64) - np.clip(ref[ok], 0, 1)
    return float(np.sqrt((d ** 2).mean())), float(ok.mean())


def test_four_lattice_frames_beat_one_full_frame(pt, oracle):
    """C3 at 160 x 90 against a 128-frame reference, display-referred (RMSE of the clamped rgb): four frames on the (0, 0) lattice of stride 2,
    filled with the albedo term off and filtered, against one full frame filtered alike; both cost one full frame of samples.
    Measured with this model: 0.0741 against 0.1138, ratio 0.651.  The bound 0.8 leaves room for small changes of the rule; the models are
    deterministic."""
    w, h = 160, 90
    wl = pt.scenes.build("C3", w, h)
    sc = oracle.Scene.from_workload(wl)
    feat = _cpu_features(oracle, wl)
    seed = pt.scenes.frame_seed
    ref, _ = _accumulate(oracle, sc, w, h, [seed(f) for f in range(5001, 5129)])
    ref = ref[..., :3] / ref[..., 3:4]
    full, fullT = _accumulate(oracle, sc, w, h, [seed(1)])
    lat, latT = _accumulate(oracle, sc, w, h, [seed(f) for f in range(1, 5)], xs=2, ys=2)
    on = lattice(h, w, 2, 0, 0)
    assert (lat[..., 3][on] == 4).all() and not lat[~on].any()
    assert _bits_equal(_accumulate(oracle, sc, w, h, [seed(1)], xs=2, ys=2)[0][on], full[on])      # a lattice pixel is the full render's
    args = (5, 2.0, 0.3, 0.05, INF, 4, 0.2)
    e_full, ok_full = _clamped_rmse(denoise_guided_demod(full, feat, fullT, *args)[..., :3], ref)
    e_lat, ok_lat = _clamped_rmse(denoise_guided_filled(lat, feat, latT, *args)[..., :3], ref)
    print(f"clamped RMSE: full {e_full:.4f}, lattice {e_lat:.4f}, ratio {e_lat / e_full:.3f}; finite {ok_full:.4f} / {ok_lat:.4f}")
    assert ok_full > 0.99 and ok_lat > 0.99
    assert e_lat / e_full < 0.8, (e_lat, e_full)
