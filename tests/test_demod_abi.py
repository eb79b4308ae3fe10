"""CPU: the albedo-demodulated surface (include/pt_demod.h) — exported symbols, a strict-C99 client, and hand cases of the float32 model
(tests/_demod_model.py) that tests/test_gpu_demod.py holds the device to."""
import ctypes
import os
import subprocess

import numpy as np

from _demod_model import carried_albedo, demodulate, denoise_guided_demod, passes, reproject_demod, select_guided_demod
from _denoise_model import classify, features
from _guided_model import denoise_guided, lum, variance
from _reproject_model import cam_rot
from _steer_model import select_guided
from test_adaptive_abi import _declared
from test_reproject_abi import H as RH
from test_reproject_abi import W as RW
from test_reproject_abi import _fin, _records
from test_reproject_abi import _frame as _rframe
from test_reproject_abi import _run as _rplain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
f32 = np.float32
NAMES = ["pt_denoise_guided_demod", "pt_read_display_denoised_guided_demod", "pt_render_adaptive_guided_demod", "pt_reproject_frame_demod",
         "pt_select_guided_demod"]
SIG = (2.0, 0.3, 0.05)                                  # the defaults' sigma_lum, sigma_normal, sigma_depth
H, W, NFR = 27, 48, 8
GREY, BLUE = f32([0.9, 0.9, 0.9]), f32([0.157, 0.235, 0.784])


def test_hip_library_exports_the_demod_symbols(pt):
    from pathtracer_0_amd import build
    lib = ctypes.CDLL(build.build_hip())
    assert _declared("pt_demod.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), n
    for other in ("pt_api.h", "pt_adaptive.h", "pt_denoise.h", "pt_reproject.h", "pt_guided.h", "pt_steer.h"):
        assert not set(NAMES) & set(_declared(other)), other


def test_demod_header_compiles_as_c99(tmp_path):
    src = tmp_path / "client.c"
    src.write_text('#include "pt_api.h"\n#include "pt_demod.h"\n#include <stddef.h>\n'
                   "int main(void) {\n"
                   "    pt_guided_rule rule = {5, 2.0f, 0.3f, 0.05f, 0.1f, 4, 0.05f, 0.0f, 0};\n"
                   "    int (*d)(pt_ctx*, int, float, float, float, float, int, float, float*) = pt_denoise_guided_demod;\n"
                   "    int (*v)(pt_ctx*, int, float, float, float, float, int, float, int, uint8_t*) = pt_read_display_denoised_guided_demod;\n"
                   "    int (*s)(pt_ctx*, const pt_guided_rule*, float, uint8_t*, int64_t*) = pt_select_guided_demod;\n"
                   "    int (*g)(pt_ctx*, int, int, const int32_t*, const pt_guided_rule*, float, int64_t*) = pt_render_adaptive_guided_demod;\n"
                   "    int (*r)(pt_ctx*, float, float, float, int, float, int64_t*) = pt_reproject_frame_demod;\n"
                   "    return (d == NULL) + (v == NULL) + (s == NULL) + (g == NULL) + (r == NULL) + (rule.iterations != 5);\n}\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "client.o")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr


# ---------------------------------------------------------------------------------------------------------------- the filter's model

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


def _relmax(a, b):
    return float(np.abs(a / b - 1).max())


def test_the_pass_loop_is_the_plain_model_s():
    """passes() repeats _guided_model.denoise_guided's loop for a given (c, v): fed the plain input, it must return the plain result bit for bit"""
    feat = _checker_feat()
    frame, T = _samples(feat[..., 4:7])
    T[3, 5, 2] = 1.0                                    # below min_frames: pooled
    for sig_a in (0.1, INF):
        want, wv = denoise_guided(frame, feat, T, 3, *SIG, sig_a, 4, return_var=True)
        c, cls = classify(frame, feat)
        got, gv = passes(c, variance(frame, feat, T, 4), cls, feat, 3, *SIG, sig_a)
        assert np.array_equal(got, want[..., :3]) and np.array_equal(gv, wv)


def test_a_uniform_albedo_gives_the_plain_result():
    """albedo 0.5 everywhere: I = 2c, T' = (2 sY, 4 sYY), every scaling by a power of two is exact, so the demodulated filter differs from the
    plain one only through the 1e-10 of e_c's denominator.  Measured 2.4e-7."""
    feat = features(H, W)                               # Kd = (0.5, 0.5, 0.5)
    frame, T = _samples(_checker_feat()[..., 4:7])
    plain = denoise_guided(frame, feat, T, 5, *SIG, 0.1, 4)
    got = denoise_guided_demod(frame, feat, T, 5, *SIG, 0.1, 4, 0.01)
    assert np.allclose(got, plain, rtol=1e-6, atol=0), _relmax(got[..., :3], plain[..., :3])


def test_a_checker_albedo_over_constant_illumination_comes_back():
    """colour = checker albedo * 0.6 without noise: the illumination is constant, so with the albedo term off the demodulated filter returns its
    input (measured 3.6e-7), where the plain filter blurs the texture (measured 4.6 %)"""
    feat = _checker_feat()
    Kd = feat[..., 4:7]
    _, T = _samples(Kd)                                 # the noise estimate of a noisy render: the filter does filter
    truth = (Kd * f32(0.6)).astype(f32)
    frame = np.concatenate([truth * f32(NFR), np.full((H, W, 1), NFR, f32)], -1).astype(f32)
    got = denoise_guided_demod(frame, feat, T, 5, *SIG, INF, 4, 0.01)
    assert np.allclose(got[..., :3], truth, rtol=1e-6, atol=0), _relmax(got[..., :3], truth)
    plain = denoise_guided(frame, feat, T, 5, *SIG, INF, 4)
    assert _relmax(plain[..., :3], truth) > 0.01


def test_demodulation_lowers_the_error_of_the_noisy_checker():
    """the CPU experiment that motivated the calls: the demodulated filter with the albedo term off beats both settings of the plain one"""
    feat = _checker_feat()
    Kd = feat[..., 4:7]
    frame, T = _samples(Kd)
    truth = Kd * f32(0.6)
    rmse = lambda o: float(np.sqrt(((o[..., :3] - truth) ** 2).mean()))      # noqa: E731
    plain = min(rmse(denoise_guided(frame, feat, T, 5, *SIG, sa, 4)) for sa in (0.1, INF))
    assert rmse(denoise_guided_demod(frame, feat, T, 5, *SIG, INF, 4, 0.01)) < plain


def _ulps(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b).astype(f32)).astype(np.float64)


def test_zero_iterations_are_within_two_ulp_of_the_mean():
    feat = _checker_feat()
    frame, T = _samples(feat[..., 4:7])
    got = denoise_guided_demod(frame, feat, T, 0, *SIG, 0.1, 4, 0.01)
    mean = frame[..., :3] / frame[..., 3:4]
    assert _ulps(got[..., :3], mean).max() <= 2.0
    assert not np.array_equal(got[..., :3], mean)       # a * (c / a): not the identity
    assert np.array_equal(got[..., 3], frame[..., 3])


def test_a_channel_below_the_floor_takes_the_floor():
    feat = features(2, 2, albedo=(0.001, 0.5, 0.0))
    frame = np.concatenate([np.full((2, 2, 3), 0.25 * 4, f32), np.full((2, 2, 1), 4.0, f32)], -1)
    T = np.zeros((2, 2, 4), f32)
    T[..., 2] = 4.0
    d = demodulate(frame, feat, T, 0.1)
    assert np.array_equal(d["a"][0, 0], f32([0.1, 0.5, 0.1]))
    assert np.array_equal(d["I"][0, 0], f32(0.25) / f32([0.1, 0.5, 0.1]))
    assert d["L"][0, 0] == lum(f32([0.1, 0.5, 0.1]))
    assert np.array_equal(carried_albedo(feat, 0.1)[0, 0], f32([0.1, 0.5, 0.1]))
    # a black albedo under a bright pixel and a tiny floor: I overflows, and the pixel is invalid (passed through as its mean)
    frame[1, 1, :3] = 4.0e30
    d = demodulate(frame, feat, T, 1e-30)
    assert d["cls"][1, 1] == 0 and d["cls"][0, 0] == 1 and np.array_equal(d["a"][1, 1], f32([1, 1, 1])) and d["L"][1, 1] == 1
    out = denoise_guided_demod(frame, feat, T, 2, *SIG, INF, 4, 1e-30)
    assert np.array_equal(out[1, 1, :3], f32([1.0e30] * 3))


def test_pixels_without_an_albedo_see_the_plain_rule():
    """an all-miss image and an image of invalid pixels: a = 1 and L = 1, bit for bit the plain model (filter and selection)"""
    frame, T = _samples(_checker_feat()[..., 4:7])
    miss = features(H, W, hit=-1)
    invalid = _checker_feat()
    invalid[..., 1] = np.nan                            # no normal
    for feat in (miss, invalid):
        for it in (0, 3):
            assert np.array_equal(denoise_guided_demod(frame, feat, T, it, *SIG, 0.1, 4, 0.01), denoise_guided(frame, feat, T, it, *SIG, 0.1, 4))
            a, da = select_guided_demod(frame, feat, T, it, *SIG, 0.1, 4, 0.05, floor=0.01, detail=True)
            b, db = select_guided(frame, feat, T, it, *SIG, 0.1, 4, 0.05, detail=True)
            assert np.array_equal(a, b) and np.array_equal(da["step"], db["step"])
    assert (classify(frame, miss)[1] == 2).all() and (classify(frame, invalid)[1] == 0).all()


def test_step_five_scales_with_the_albedo():
    """a uniform grey albedo and the colour multiplied by the same factor: I, T' and v_K stay, (v_K L) L and tol^2 both take the factor squared
    (exactly, for a power of two), and the mask is unchanged.  Without the L^2 the mask would follow the albedo."""
    base = features(H, W, albedo=(0.5, 0.5, 0.5))
    frame, T = _samples(base[..., 4:7], noise=0.05)
    masks = []
    for k in (1.0, 0.5, 0.125):
        feat = features(H, W, albedo=(0.5 * k,) * 3)
        fr = frame.copy()
        fr[..., :3] *= f32(k)
        Tk = T.copy()
        Tk[..., 0] *= f32(k)
        Tk[..., 1] *= f32(k * k)
        act, d = select_guided_demod(fr, feat, Tk, 2, *SIG, INF, 4, 0.0032, floor=0.01, detail=True)      # the median of sqrt(v_K) / l(c_K)
        assert (d["step"] == 5).all()
        masks.append(act)
    assert 0.1 * H * W < masks[0].sum() < 0.9 * H * W    # a real selection
    assert np.array_equal(masks[0], masks[1]) and np.array_equal(masks[0], masks[2])


# ---------------------------------------------------------------------------------------------------------------- the reprojection's model

def _rdemod(rn, rh, fr, fin_h, fin_n, T=None, mh=64.0, floor=0.01):
    return reproject_demod(rn, rh, fr, T, fin_h, fin_n, np.array((0,), np.uint8), cam_rot(fin_h["rotation"]), mh, 0.02, 0.9, False, floor)


def _albedo_columns(rec):
    """Kd of column x: grey on even columns, blue on odd ones; the misses keep zeros"""
    rec = rec.copy()
    hit = np.ascontiguousarray(rec[..., 7]).view(np.int32) != -1
    xx = np.broadcast_to(np.arange(RW)[None, :], (RH, RW))
    rec[..., 4:7] = np.where((xx % 2 == 0)[..., None], GREY, BLUE)
    rec[~hit, 4:7] = 0.0
    return rec


def test_reprojection_with_an_unchanged_camera_is_the_identity():
    fin = _fin()
    rec = _albedo_columns(_records(fin, miss_cols=(0,)))
    fr = _rframe()
    T = np.concatenate([fr[..., :2], np.full((RH, RW, 1), 3.0, f32), np.zeros((RH, RW, 1), f32)], -1)
    out, tout, kept = _rdemod(rec, rec, fr, fin, fin, T)
    assert kept == RW * RH
    assert np.array_equal(out.view(np.uint32), fr.view(np.uint32)) and np.array_equal(tout.view(np.uint32), T.view(np.uint32))
    # ... and under the cap it is the plain call
    want, wantT, _ = _rplain(rec, rec, fr, fin, fin, T, mh=2.0)
    out, tout, _ = _rdemod(rec, rec, fr, fin, fin, T, mh=2.0)
    assert np.array_equal(out, want) and np.array_equal(tout, wantT)


def test_a_one_pixel_shift_over_two_albedos_exchanges_them():
    """the move of test_translation_facing_a_plane_shifts_by_whole_pixels: new pixel x is old pixel x - 1, whose albedo is the other one"""
    fin_h, fin_n = _fin(), _fin(origin=(1.0, 0.0, 0.0))
    rh, rn = _albedo_columns(_records(fin_h)), _albedo_columns(_records(fin_n))
    fr = _rframe(count=100.0)
    T = np.zeros((RH, RW, 4), f32)
    T[..., 0], T[..., 1], T[..., 2] = 30.0, 90.0, 50.0
    out, tout, kept = _rdemod(rn, rh, fr, fin_h, fin_n, T, mh=1000.0)
    assert kept == (RW - 1) * RH and not out[:, 0].any() and not tout[:, 0].any()
    bn, bh = carried_albedo(rn, 0.01)[:, 1:], carried_albedo(rh, 0.01)[:, :-1]
    assert np.array_equal(bn[0, 0], BLUE) and np.array_equal(bh[0, 0], GREY)
    assert np.array_equal(out[:, 1:, :3], fr[:, :-1, :3] * (bn / bh)) and np.array_equal(out[:, 1:, 3], fr[:, :-1, 3])
    rho = lum(bn) / lum(bh)
    assert np.array_equal(tout[:, 1:, 0], f32(30.0) * rho) and np.array_equal(tout[:, 1:, 1], (f32(90.0) * rho) * rho)
    assert (tout[:, 1:, 2] == 50.0).all()
    # the caps come after the scaling
    out, tout, _ = _rdemod(rn, rh, fr, fin_h, fin_n, T, mh=10.0)
    f, g = f32(10.0) / f32(100.0), f32(10.0) / f32(50.0)
    assert np.array_equal(out[:, 1:, :3], (fr[:, :-1, :3] * (bn / bh)) * f) and (out[:, 1:, 3] == 10.0).all()
    assert np.array_equal(tout[:, 1:, 0], (f32(30.0) * rho) * g) and np.array_equal(tout[:, 1:, 1], ((f32(90.0) * rho) * rho) * g)
    # a floor above the blue albedo's red and green channels
    out, _, _ = _rdemod(rn, rh, fr, fin_h, fin_n, None, mh=1000.0, floor=0.5)
    lo = np.maximum(BLUE, f32(0.5))
    assert np.array_equal(out[0, 1, :3], fr[0, 0, :3] * (lo / GREY)) and np.array_equal(out[0, 2, :3], fr[0, 1, :3] * (GREY / lo))
