"""CPU: the float32 models of the guided filter (tests/_guided_model.py) and of its demodulated form (tests/_demod_model.py) against the float64
reference of tests/_guided_ref64.py, within the per-pixel bound that module derives, on synthetic frames, feature records and moments; the same
comparison failing by far for models with one rule of include/pt_guided.h or include/pt_demod.h misread, so that the bound is known to be tight
enough to catch such a misreading on the device (tests/test_gpu_guided_ref.py); hand cases for the reference alone; and the share of pixels whose
bound says nothing kept at or below 2 % on every input.

Degenerate depths.  The header divides by t_p.  A hit with a denormal t_p keeps (t_p - t_p) / t_p = 0 at its own tap and loses every other tap
(the quotient overflows), so it passes through: the float32 model, which divides, agrees with the reference.  A kernel that multiplies by 1 / t_p
instead has 1 / t_p = +inf there and 0 * inf = NaN at the pixel's own tap: it is on the other side.  A hit with t_p = 0 is NaN by
the header itself (0 / 0), and from the next pass on so is every pixel that takes it as a tap while the luminance term is on; such a pixel is kept
out of the main inputs, where it would leave nothing to compare, and has a test of its own."""
import os
import types

import numpy as np
import pytest

import _demod_model
import _guided_model
import _guided_ref64 as ref64
from _denoise_model import features
from test_gpu_guided import CASES

INF = float("inf")
f32 = np.float32
# the five parameter sets of tests/test_gpu_guided.py's CASES as (sigmas, min_frames, the albedo floor each runs with in the demodulated form)
FLOORS = (0.01, 0.05, 0.85, 0.01, 1e-3)
PARAMS = [(sig, mf, floor) for (_, sig, mf), floor in zip(CASES, FLOORS)]
assert len(PARAMS) == len(CASES) == 5
KS = (0, 1, 3, 8)
SHAPES = [(23, 37), (1, 1), (1, 13), (13, 1), (5, 70), (40, 9)]
SETS = ("noisy", "n8", "converged")
CAP = 0.02


def synthetic_features(H, W, seed=1, zero_t=False):
    """feature records: varying depth and normals, a textured albedo, materials in vertical bands, a block of misses and scattered ones, a NaN
    normal, an infinite depth, a hit with a denormal t; zero_t: also a hit with t = 0"""
    rs = np.random.RandomState(seed)
    feat = features(H, W)
    feat[..., 0] = (0.5 + 2.5 * rs.rand(H, W)).astype(f32)
    n = rs.randn(H, W, 3).astype(f32) * f32(0.3) + np.array([0.0, 1.0, 0.0], f32)
    feat[..., 1:4] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    feat[..., 4:7] = np.where((np.arange(W) < W // 2)[None, :, None], f32(0.3), f32(0.7)) + rs.rand(H, W, 3).astype(f32) * f32(0.25)
    miss = rs.rand(H, W) < 0.15
    miss[: H // 3, : W // 4] = True
    band = np.broadcast_to(np.arange(W)[None, :] // 5, (H, W))
    feat[..., 7] = np.where(miss, -1, 0x1000000 + band).astype(np.int32).view(f32)
    feat[..., 11] = np.where(miss, -1, band % 3).astype(np.int32).view(f32)
    feat[miss, 0] = -1.0
    feat[miss, 1:7] = 0.0
    if H > 4 and W > 6:
        feat[4, 5, 2] = np.nan
        feat[H - 1, W - 1, 0] = np.inf
        for y, x, t in ((H - 2, W - 3, 1e-40),) + (((H // 2, W // 2, 0.0),) if zero_t else ()):
            feat[y, x] = feat[0, W - 1]
            feat[y, x, 0] = t
            feat[y, x, 7] = np.array([0x1000000], np.int32).view(f32)[0]
            feat[y, x, 11] = np.array([0], np.int32).view(f32)[0]
    return feat


def frame_for(feat, seed=3):
    """FRAME over given feature records: counts 1 .. 8; an illumination times the pixel's Kd (1 on a miss), as a diffuse first hit renders it and
    as include/pt_demod.h assumes.  The left half is a detailed illumination without noise (two crossed waves, noise of a few 1e-4 relative),
    the right half one scattered by +-0.25 around 0.6; NaN and infinite means and a never-rendered pixel with colour.
    The cap decides this form.  On a surface where nothing but the luminance term stops a tap (a wall), 8 passes at sigma_lum 10 divide v by
    about ten each, so sqrt(g_p) falls a thousandfold.  Colour differences far above that are weighed by rounding, and the pixel is
    uninformative.  So the scatter of the right half is what the moments of moments_for() describe (a per-frame variance around 0.1 over a few
    frames), not several times that; the colour follows Kd, because means independent of a coloured Kd demodulate into chroma scatter several
    times the luminance scatter the weights see; and the left half has the detail a converged image has, which cuts its far taps by luminance
    as the filter means them to be cut (DESIGN.md 2.10 says how much of that half is still filtered)."""
    H, W = feat.shape[:2]
    rs = np.random.RandomState(seed)
    cnt = rs.randint(1, 9, size=(H, W, 1)).astype(f32)
    noisy = (0.35 + 0.5 * rs.rand(H, W, 3)).astype(f32)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = 0.6 + 0.2 * np.sin(0.9 * xx + 0.53 * yy) + 0.15 * np.sin(0.23 * xx - 1.1 * yy)
    miss = np.ascontiguousarray(feat[..., 7]).view(np.int32) == -1
    kd = np.where(miss[..., None], 1.0, np.where(np.isfinite(feat[..., 4:7]), feat[..., 4:7], 0.0))
    light = np.where((xx < (W + 1) // 2)[..., None], ramp[..., None] * (1.0 + 3e-4 * rs.randn(H, W, 3)), noisy)
    mean = (kd * light).astype(f32)                                       # colour = Kd * illumination, as a diffuse first hit renders it
    frame = np.concatenate([mean * cnt, cnt], -1).astype(f32)
    if H > 4 and W > 6:
        frame[1, 2] = (3.0, 4.0, 5.0, 0.0)                        # never rendered
        frame[2, 3, 1] = np.nan
        frame[3, 4, :3] = np.inf
    return frame


def moments_for(kind, frame, seed=7):
    """T over a given FRAME.  noisy: the recipe of tests/test_gpu_guided.py's _inject at any size (the same array at 96x54): n = 0 .. 8
    independent of FRAME.a, random sums, a NaN sum, and one more NaN sum on a pixel with n = 8.  n8: the same with every n >= 8 and finite sums.
    converged: on the left half n = 8 .. 15 frames around the pixel's own luminance with a per-frame relative standard deviation around 1e-3,
    noisy on the right half."""
    H, W = frame.shape[:2]
    rs = np.random.RandomState(seed)
    rs.randint(1, 9, size=(H, W, 1)); rs.rand(H, W, 3)                     # _inject draws its FRAME first
    n = rs.randint(0, 9, size=(H, W)).astype(f32)
    Y = rs.rand(H, W).astype(f32)
    sY = (n * Y).astype(f32)
    sYY = (n * Y * Y * (1.0 + rs.rand(H, W) * 0.5)).astype(f32)
    T = np.stack([sY, sYY, n, np.zeros_like(n)], -1).astype(f32)
    y, x = min(40, H - 1), min(50, W - 1)
    y2, x2 = H // 2, (3 * W) // 4
    T[y, x, :2] = np.nan
    T[y2, x2] = (np.nan, np.nan, 8.0, 0.0)                                  # (one more than _inject has: own moments that give no estimate)
    if kind == "noisy":
        return T
    T[..., 2] = np.maximum(T[..., 2], 8.0)
    T[y, x, :2] = (4.0, 3.0)
    T[y2, x2, :2] = (4.0, 3.0)
    if kind == "n8":
        return T
    assert kind == "converged"
    with np.errstate(all="ignore"):
        mean = frame[..., :3].astype(np.float64) / frame[..., 3:4]
    Yc = np.nan_to_num(ref64.lum64(mean), nan=0.5, posinf=0.5, neginf=0.5)
    nc = rs.randint(8, 16, size=(H, W)).astype(np.float64)
    s = 1e-3 * Yc * (0.5 + rs.rand(H, W))
    Tc = np.stack([nc * Yc, nc * Yc * Yc + (nc - 1) * s * s, nc, np.zeros((H, W))], -1).astype(f32)
    left = (np.mgrid[0:H, 0:W][1] < (W + 1) // 2)[..., None]
    return np.where(left, Tc, T).astype(f32)


def synthetic(H, W, kind="noisy", zero_t=False):
    feat = synthetic_features(H, W, zero_t=zero_t)
    frame = frame_for(feat)
    T = moments_for(kind, frame)
    if kind == "noisy" and H > 4 and W > 6:                                  # a hit of a material of its own below min_frames: nothing to pool with
        y, x = H // 2 + 1, W // 3
        feat[y, x] = feat[0, W - 1]
        feat[y, x, 7] = np.array([0x1000000], np.int32).view(f32)[0]
        feat[y, x, 11] = np.array([77], np.int32).view(f32)[0]
        T[y, x] = (0.3, 0.09, 1.0, 0.0)
    return frame, feat, T


def model_plain(frame, feat, T, K, sig, mf, floor, model=_guided_model.denoise_guided):
    out, v = model(frame, feat, T, K, *sig, mf, return_var=True)
    return out, v


def model_demod(frame, feat, T, K, sig, mf, floor, mod=_demod_model):
    I, v, d = mod.filtered_demod(frame, feat, T, K, *sig, mf, floor)
    return mod.denoise_guided_demod(frame, feat, T, K, *sig, mf, floor), v


def worst_of(run, frame, feat, T, sig, mf, floor, demod, ks=KS):
    """per pass count: (colour deviation, where, variance deviation, where, uninformative share)"""
    refs = ref64.filter64(frame, feat, T, tuple(ks), *sig, mf, floor if demod else None)
    res = {}
    for K in ks:
        out, v = run(frame, feat, T, K, sig, mf, floor)
        res[K] = ref64.deviation(out, refs[K]) + ref64.deviation_v(v, refs[K]) + (ref64.uninformative_share(refs[K]),)
    return res


@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_float32_models_within_the_bound(H, W, kind):
    frame, feat, T = synthetic(H, W, kind)
    top = [0.0, 0.0, 0.0]
    for sig, mf, floor in PARAMS:
        for demod, run in ((False, model_plain), (True, model_demod)):
            for K, (dc, at, dv, atv, share) in worst_of(run, frame, feat, T, sig, mf, floor, demod).items():
                assert dc <= 1.0, (H, W, kind, sig, mf, demod, K, dc, at)
                assert dv <= 1.0, (H, W, kind, sig, mf, demod, K, dv, atv)
                assert share <= CAP, (H, W, kind, sig, mf, demod, K, share)          # the cap: a condition on the input
                top = [max(a, b) for a, b in zip(top, (dc, dv, share))]
    print(f"guided model {H}x{W} {kind}: colour {top[0]:.4f} and variance {top[1]:.4f} of the bound, uninformative {top[2]:.4f}")


def test_degenerate_depths():
    """a hit with t = 0 (NaN by the header, spreading through the luminance term) beside the denormal one: the model and the reference agree on
    which pixels are NaN and on every other pixel"""
    frame, feat, T = synthetic(23, 37, "noisy", zero_t=True)
    for sig, mf, floor in PARAMS:
        refs = ref64.filter64(frame, feat, T, (1, 3), *sig, mf)
        for K in (1, 3):
            out, v = model_plain(frame, feat, T, K, sig, mf, floor)
            assert ref64.deviation(out, refs[K])[0] <= 1.0, (sig, K)
            assert np.isnan(refs[K]["out"][23 // 2, 37 // 2, :3]).all()
            assert np.isfinite(refs[K]["out"][21, 34, :3]).all()                      # the denormal t: passed through
            assert np.array_equal(refs[K]["out"][21, 34, :3], (frame[21, 34, :3] / frame[21, 34, 3]).astype(np.float64))


def _one(frame, feat, T, K, sig=(1.0, INF, INF, INF), mf=2, floor=None):
    return ref64.filter64(frame, feat, T, K, *sig, mf, floor)


def test_the_reference_on_hand_cases():
    # a single valid pixel: itself, whatever the passes; v = s2 / A carried as (w^2 v) / w^2
    frame = np.array([[[1.0, 2.0, 3.0, 4.0]]], f32)
    T = np.array([[[4.0, 6.0, 4.0, 0.0]]], f32)                              # m = 1, s2 = (6 - 4) / 3
    for K in (0, 5):
        r = _one(frame, features(1, 1), T, K)
        assert np.array_equal(r["out"], [[[0.25, 0.5, 0.75, 4.0]]])
        assert abs(r["v"][0, 0] - float(f32(f32(2.0) / f32(3.0)) / f32(4.0))) < 1e-14
        assert r["bound_c"].max() <= 64 * 5 * ref64.U and ref64.uninformative_share(r) == 0.0
    frame[0, 0, 3] = 0.0                                                     # never rendered: its raw rgb
    assert np.array_equal(_one(frame, features(1, 1), T, 3)["out"], [[[1.0, 2.0, 3.0, 0.0]]])
    # two pixels of a row with known v: grey 0.25 and 0.75 at A = 4, v = (0.04, 0.16) / 4 (float32 moments chosen exactly representable)
    frame = np.array([[[1.0, 1.0, 1.0, 4.0], [3.0, 3.0, 3.0, 4.0]]], f32)
    T = np.array([[[4.0, 4.0 + 3 * 0.25, 4.0, 0.0], [4.0, 4.0 + 3 * 1.0, 4.0, 0.0]]], f32)     # s2 = 0.25 and 1
    v = np.array([0.25 / 4, 1.0 / 4])
    r = _one(frame, features(1, 2), T, 1, sig=(2.0, INF, INF, INF))
    lsum = sum(ref64.LC)
    g = (0.5 * v + 0.25 * v[::-1]) / 0.75
    e = abs(0.25 * lsum - 0.75 * lsum) / (2.0 * np.sqrt(g) + 1e-10)
    w = np.exp(-e)
    c = np.array([0.25, 0.75])
    want_c = (6 * c + 4 * w * c[::-1]) / (6 + 4 * w)
    want_v = (36 * v + 16 * w * w * v[::-1]) / (6 + 4 * w) ** 2
    assert np.abs(r["out"][0, :, 0] - want_c).max() < 1e-14 and np.abs(r["v"][0] - want_v).max() < 1e-14
    # a tap with v = +inf: pixel 2 has n = 1 < min_frames and a material of its own, so it pools N = 1: no estimate.  Pass 0: g_1 and g_2 are +inf
    # (their 3x3 holds pixel 2), so pixels 1 and 2 weigh their taps with the bare B3 weights; g_0 is finite and pixel 0 weighs by luminance; all
    # three take pixel 2, so every v' is +inf.  Pass 1 (step 2): g_0 is +inf now, and pixel 0 takes pixel 2 at 4/16 against its own 6/16.
    c = np.array([0.25, 0.75, 0.5])
    frame = np.stack([np.concatenate([np.full(3, 4 * x, f32), [f32(4.0)]]) for x in c])[None]
    feat = features(1, 3)
    feat[0, 2, 11] = np.array([5], np.int32).view(f32)[0]
    T = np.array([[[4.0, 4.75, 4.0, 0.0], [4.0, 7.0, 4.0, 0.0], [1.0, 1.0, 1.0, 0.0]]], f32)
    r1 = _one(frame, feat, T, 1)
    assert np.isinf(r1["v"][0]).all() and not r1["bound_v"][0].any()
    g0 = (0.5 * v[0] + 0.25 * v[1]) / 0.75
    w1, w2 = (np.exp(-abs(c[0] - x) * lsum / (np.sqrt(g0) + 1e-10)) for x in c[1:])
    want = [(6 * c[0] + 4 * w1 * c[1] + w2 * c[2]) / (6 + 4 * w1 + w2), (4 * c[0] + 6 * c[1] + 4 * c[2]) / 14, (c[0] + 4 * c[1] + 6 * c[2]) / 11]
    c1 = r1["out"][0, :, 0]
    assert np.abs(c1 - want).max() < 1e-14
    r2 = _one(frame, feat, T, 2)
    assert abs(r2["out"][0, 0, 0] - (6 * c1[0] + 4 * c1[2]) / 10) < 1e-14 and abs(r2["out"][0, 1, 0] - c1[1]) < 1e-14
    # a pixel below min_frames with exactly two poolable neighbours: S, Q, N over the three, s2 = (Q - S*(S/N)) / (N - 1) in float32
    frame = np.tile(np.array([2.0, 2.0, 2.0, 2.0], f32), (1, 4, 1))
    feat = features(1, 4)
    feat[0, 3, 11] = np.array([9], np.int32).view(f32)[0]                   # another material: not pooled
    T = np.array([[[1.0, 1.5, 1.0, 0.0], [0.5, 0.25, 1.0, 0.0], [3.0, 5.0, 2.0, 0.0], [7.0, 50.0, 3.0, 0.0]]], f32)
    r = _one(frame, feat, T, 0, mf=4)
    S, Q, N = f32(1.0) + f32(0.5) + f32(3.0), f32(1.5) + f32(0.25) + f32(5.0), f32(4.0)
    s2 = f32(f32(Q - f32(S * f32(S / N))) / f32(N - f32(1.0)))
    assert r["v"][0, 0] == float(f32(s2 / f32(2.0))) and r["v"][0, 0] == r["v"][0, 1] == r["v"][0, 2]
    assert np.array_equal(r["out"], frame.astype(np.float64) / [2.0, 2.0, 2.0, 1.0])   # iterations 0: the identity


# one misreading of include/pt_guided.h (or, "demod_", of include/pt_demod.h) each, applied to the float32 model's text.
# (The luminance term left on where g_p = +inf cannot be told from the rule as a misreading of the division itself: x / (sigma*sqrt(inf) + 1e-10)
# is 0 as well.  It shows when g_p is not +inf where it should be: the mutant below forms g_p from the finite v_q alone.)
MUTATIONS = {
    "v_with_w": ("sv + (w * w) * vq", "sv + w * vq"),
    "v_over_sum_w_once": ("sv / (sw * sw)", "sv / sw"),
    "g_not_normalised": ("g = gs / gw", "g = gs"),
    "pool_across_materials": (" & ((cls != 1) | (_shift(mat, dy, dx, -1) == mat))", ""),
    "s2_over_n": ("v = (s2 / frame[..., 3])", "v = (s2 / n)"),
    "lum_on_where_g_inf": ("use = valid & (_shift(cls, dy, dx, 0) == cls)\n", "use = valid & (_shift(cls, dy, dx, 0) == cls) & (_shift(v, dy, dx, np.float32(0)) != INF32)\n"),
    "step_not_on_dy": ("ddy, ddx = dy * s, dx * s", "ddy, ddx = dy, dx * s"),
    "clamp_out_of_image_taps": ("    H, W = a.shape[:2]\n    out = np.full_like(a, fill)\n",
                                "    H, W = a.shape[:2]; yy, xx = np.mgrid[0:H, 0:W]; return a[np.clip(yy + dy, 0, H - 1), np.clip(xx + dx, 0, W - 1)]\n"),
    "demod_pool_over_centre_L": ('v = variance(frame, d["feat"], d["T"], min_frames)',
                                 'v = (variance(frame, d["feat"], np.asarray(T, f32), min_frames) / (d["L"] * d["L"])).astype(f32)'),
}


def _mutant(name):
    old, new = MUTATIONS[name]
    demod = name.startswith("demod_")
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "_demod_model.py" if demod else "_guided_model.py")).read()
    assert src.count(old) == 1, name
    mod = types.ModuleType("_guided_mutant_" + name)
    exec(compile(src.replace(old, new), mod.__name__, "exec"), mod.__dict__)
    if demod:
        return lambda *a: model_demod(*a, mod=mod)
    return lambda *a: model_plain(*a, model=mod.denoise_guided)


def _finite_excess(got, ref):
    """the largest |got - ref| / bound over the values finite on both sides: what deviation() gives without its +inf for a mismatched NaN or infinity"""
    g, w, b = np.asarray(got, np.float64)[..., :3], ref["out"][..., :3], ref["bound_c"]
    ok = np.isfinite(g) & np.isfinite(w) & np.isfinite(b) & (b > 0)
    return float((np.abs(g[ok] - w[ok]) / b[ok]).max()) if ok.any() else 0.0


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutated_models_fail_the_bound(name):
    bad = _mutant(name)
    demod = name.startswith("demod_")
    worst = finite = 0.0
    for kind in ("noisy", "converged"):
        frame, feat, T = synthetic(23, 37, kind)
        for sig, mf, floor in PARAMS:
            refs = ref64.filter64(frame, feat, T, (1, 3), *sig, mf, floor if demod else None)
            for K in (1, 3):
                out, _ = bad(frame, feat, T, K, sig, mf, floor)                       # the colour alone: what the device's output shows
                worst = max(worst, ref64.deviation(out, refs[K])[0])
                finite = max(finite, _finite_excess(out, refs[K]))
    assert worst > 1.0, (name, worst)
    # ... and by a wide margin, in finite values (a mismatched infinity alone would say nothing about the bound): it is not the reason they fail narrowly
    assert finite > 100.0, (name, finite, worst)
