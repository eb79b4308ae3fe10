"""CPU: reprojection with bilinear taps (include/pt_reproject_bilinear.h) — the exported symbol, a strict-C99 client, hand cases of the float32 model
(tests/_reproject_bilinear_model.py) that tests/test_gpu_reproject_bilinear.py holds the device to, and the oracle experiment the call rests on."""
import ctypes
import glob
import os
import subprocess

import numpy as np

from _demod_model import reproject_demod
from _reproject_bilinear_model import reproject_bilinear
from _reproject_model import cam_rot, material_flags, overlay, reproject
from test_adaptive_abi import _declared
from test_fill_abi import _accumulate, _bits_equal, _cpu_features
from test_motion_abi import _random_case
from test_reproject_abi import H, W, _fin, _frame, _records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ["pt_reproject_frame_bilinear"]
SNAP = 1.0 / 64


def test_hip_library_exports_the_bilinear_symbol(pt):
    from pathtracer_0_amd import build
    lib = ctypes.CDLL(build.build_hip())
    assert _declared("pt_reproject_bilinear.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), n
    others = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "pt_reproject_bilinear.h")
    assert "pt_reproject.h" in others and "pt_demod.h" in others
    for other in others:
        assert not set(NAMES) & set(_declared(other)), other


def test_bilinear_header_compiles_as_c99(tmp_path):
    src = tmp_path / "client.c"
    src.write_text('#include "pt_api.h"\n#include "pt_reproject_bilinear.h"\n#include <stddef.h>\n'
                   "int main(void) {\n"
                   "    int64_t kept = 0, blended = 0;\n"
                   "    pt_reproject_bilinear_rule r;\n"
                   "    int (*f)(pt_ctx*, const pt_reproject_bilinear_rule*, int64_t*, int64_t*) = pt_reproject_frame_bilinear;\n"
                   "    r.max_history = 64.0f; r.depth_tol = 0.02f; r.normal_tol = 0.9f; r.snap = 1.0f / 64.0f; r.albedo_floor = 0.0f;\n"
                   "    r.flags = PT_REPROJECT_ALL_MATERIALS;\n"
                   "    return (f == NULL) + (int)kept + (int)blended + (r.flags != 1) + (sizeof r != 24);\n}\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "client.o")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr


def test_python_rule_has_the_header_layout(pt):
    from pathtracer_0_amd import renderer
    R = renderer.ReprojectBilinearRule
    assert [n for n, _ in R._fields_] == ["max_history", "depth_tol", "normal_tol", "snap", "albedo_floor", "flags"] and ctypes.sizeof(R) == 24


# ---------------------------------------------------------------------------------------------------------------- hand cases of the model

def _run(rn, rh, fr, fin_h, fin_n, T=None, vd=(0,), mh=64.0, dt=0.25, nt=0.9, snap=SNAP, allm=False, floor=0.0):
    """depth_tol 0.25: across this 8-pixel, 90-degree view the distance to the plane changes by up to 14 % from one pixel to the next"""
    return reproject_bilinear(rn, rh, fr, T, fin_h, fin_n, np.array(vd, np.uint8), cam_rot(fin_h["rotation"]), mh, dt, nt, snap, allm, floor, detail=True)


def _moments(fr, n=3.0):
    return np.concatenate([fr[..., :2], np.full((H, W, 1), n, f32), np.zeros((H, W, 1), f32)], -1).astype(f32)


def _mean(fr):
    with np.errstate(all="ignore"):
        return fr[..., :3].astype(np.float64) / fr[..., 3:4]


def _shifted(dx, dy=0.0, **kw):
    """the plane z = 4 of _records seen from the image's camera at the origin and from a camera moved by (dx, dy) pixels' worth: a new pixel's
    point projects to (px + 0.5 - dx, py + 0.5 + dy) in the old image (one pixel is 1.0 wide on the plane; world +x is image -x, +y is +y)"""
    fin_h, fin_n = _fin(), _fin(origin=(dx, dy, 0.0), **kw)
    return _records(fin_n), _records(fin_h), fin_h, fin_n


def test_identity_camera_is_the_nearest_models_bit_for_bit():
    fin = _fin()
    for seed in (1, 2):
        rs = np.random.RandomState(seed)
        rec = _records(fin, miss_cols=(6,))
        rec[..., 4:7] = rs.rand(H, W, 3)
        fr = _frame(count=100.0, seed=seed)
        fr[0, 0, 3] = 5.0
        fr[1, 1, 0], fr[2, 2, 3], fr[3, 3, 1] = np.nan, 0.0, np.inf
        T = (rs.rand(H, W, 4) * 90).astype(f32)
        vd, M = np.array([0], np.uint8), cam_rot(fin["rotation"])
        for mh in (64.0, 10.0):
            want = reproject(rec, rec, fr, T, fin, fin, vd, M, mh, 0.02, 0.9)
            got = _run(rec, rec, fr, fin, fin, T, mh=mh)
            assert got[2] == want[2] == W * H - 3 and got[3] == 0 and _bits_equal(got[0], want[0]) and _bits_equal(got[1], want[1])
            want = reproject_demod(rec, rec, fr, T, fin, fin, vd, M, mh, 0.02, 0.9, False, 0.2)
            got = _run(rec, rec, fr, fin, fin, T, mh=mh, floor=0.2)
            assert got[2] == want[2] and got[3] == 0 and _bits_equal(got[0], want[0]) and _bits_equal(got[1], want[1])
        assert _run(rec, rec, fr, fin, fin, None)[1] is None


def test_half_pixel_shift_blends_two_taps_half_and_half():
    rn, rh, fin_h, fin_n = _shifted(0.5)
    fr = _frame(count=8.0)
    T = _moments(fr, 8.0)
    out, tout, kept, blended, d = _run(rn, rh, fr, fin_h, fin_n, T)
    assert kept == W * H and blended == (W - 1) * H
    assert (d["taps"][:, 1:] == 2).all() and (d["taps"][:, 0] == 1).all()
    w = d["weights"]
    assert np.abs(w[0][:, 1:] - 0.5).max() < 1e-5 and np.abs(w[1][:, 1:] - 0.5).max() < 1e-5 and not w[2].any() and not w[3].any()
    m = _mean(fr)
    assert np.abs(_mean(out)[:, 1:] - 0.5 * (m[:, :-1] + m[:, 1:])).max() < 1e-5 and (out[:, 1:, 3] == 8.0).all()
    ym = T[..., :2].astype(np.float64) / 8.0
    assert np.abs(tout[:, 1:, :2] / 8.0 - 0.5 * (ym[:, :-1] + ym[:, 1:])).max() < 1e-5 and (tout[:, 1:, 2] == 8.0).all() and not tout[..., 3].any()
    # column 0: its left tap is column -1, so it has its nearest neighbour alone and is a bit-exact copy
    assert _bits_equal(out[:, 0], fr[:, 0]) and _bits_equal(tout[:, 0], T[:, 0])
    # the demodulated form on a grey albedo that changes from the old pixel to the new: the mean follows the ratio
    rn2, rh2 = rn.copy(), rh.copy()
    rn2[..., 4:7], rh2[..., 4:7] = 0.5, 0.25
    out2 = _run(rn2, rh2, fr, fin_h, fin_n, floor=0.01)[0]
    assert np.abs(_mean(out2)[:, 1:] - 2.0 * 0.5 * (m[:, :-1] + m[:, 1:])).max() < 1e-5


def test_an_exact_mean_and_count_stay_exact():
    """(0.5, 0.25, 1) x 8 on every old pixel: every weight sum scales by a power of two, so every kept pixel is that mean and count bit for bit"""
    rn, rh, fin_h, fin_n = _shifted(0.3, 0.2)
    fr = np.tile(np.array([4.0, 2.0, 8.0, 8.0], f32), (H, W, 1))
    T = np.tile(np.array([4.0, 2.0, 8.0, 0.0], f32), (H, W, 1))
    out, tout, kept, blended, d = _run(rn, rh, fr, fin_h, fin_n, T)
    assert kept == W * H and blended == W * H - 1 and d["taps"].max() == 4 and (d["taps"][:-1, 1:] == 4).all()
    assert _bits_equal(out, fr)
    assert _bits_equal(tout[d["taps"] >= 2], T[d["taps"] >= 2]) and _bits_equal(tout, T)


def test_a_failing_tap_leaves_the_others_renormalised():
    rn, rh, fin_h, fin_n = _shifted(0.3, 0.2)                   # taps (px - 1, py), (px, py), (px - 1, py + 1), (px, py + 1); weights .3*.8 .7*.8 .3*.2 .7*.2
    fr = _frame(count=8.0)
    m = _mean(fr)
    wts = np.array([0.3 * 0.8, 0.7 * 0.8, 0.3 * 0.2, 0.7 * 0.2])

    def want(px, py, use):
        taps = [(py, px - 1), (py, px), (py + 1, px - 1), (py + 1, px)]
        return sum(wts[k] * m[taps[k]] for k in use) / sum(wts[k] for k in use)
    base, _, kept, _, d = _run(rn, rh, fr, fin_h, fin_n)
    assert kept == W * H and np.abs(_mean(base)[2, 3] - want(3, 2, (0, 1, 2, 3))).max() < 1e-5
    assert np.abs(d["weights"][:, 2, 3] - wts).max() < 1e-5
    for what in ("depth", "normal", "material", "miss"):
        bad = rh.copy()
        if what == "depth":
            bad[2, 2, 0] *= f32(2.0)
        elif what == "normal":
            bad[2, 2, 1:4] = (0.0, -0.6, -0.8)
        elif what == "material":
            bad[2, 2, 11] = np.array([1], np.int32).view(f32)[0]
        else:
            bad[2, 2, 7] = np.array([-1], np.int32).view(f32)[0]
        out, _, kept, _, d = _run(rn, bad, fr, fin_h, fin_n, vd=(0, 0))
        assert kept == W * H, what
        # old pixel (2, 2) is tap 0 of new (3, 2), tap 1 of (2, 2), tap 2 of (3, 1), tap 3 of (2, 1)
        for (px, py), k in (((3, 2), 0), ((2, 2), 1), ((3, 1), 2), ((2, 1), 3)):
            use = [t for t in range(4) if t != k]
            assert d["taps"][py, px] == 3 and not d["counts"][k, py, px], (what, px, py)
            assert np.abs(_mean(out)[py, px] - want(px, py, use)).max() < 1e-5, (what, px, py)
            assert abs(float(out[py, px, 3]) - 8.0) < 1e-5
        other = np.ones((H, W), bool)
        for py, px in ((2, 3), (2, 2), (1, 3), (1, 2)):
            other[py, px] = False
        assert _bits_equal(out[other], base[other]), what
    # a new pixel that is a miss takes miss taps only, a hit none of them
    rn_m, rh_m = rn.copy(), _records(fin_h, miss_cols=(4,))
    out, _, kept, _, d = _run(rn_m, rh_m, fr, fin_h, fin_n)
    assert (d["taps"][1:-1, 4] == 2).all() and (d["taps"][1:-1, 5] == 2).all() and not d["counts"][1][:, 4].any() and not d["counts"][0][:, 5].any()


def test_taps_off_the_image_borders():
    fr = _frame(count=8.0)
    T = _moments(fr, 8.0)
    # +0.25: fx = px - 0.25, taps px - 1 (0.25) and px (0.75); column 0 has ix = -1
    rn, rh, fin_h, fin_n = _shifted(0.25)
    out, tout, kept, blended, d = _run(rn, rh, fr, fin_h, fin_n, T)
    assert kept == W * H and blended == (W - 1) * H and (d["taps"][:, 0] == 1).all()
    assert _bits_equal(out[:, 0], fr[:, 0]) and _bits_equal(tout[:, 0], T[:, 0])
    # -0.25: taps px (0.75) and px + 1 (0.25); column W - 1 has ix + 1 = W
    rn, rh, fin_h, fin_n = _shifted(-0.25)
    out, tout, kept, blended, d = _run(rn, rh, fr, fin_h, fin_n, T)
    assert kept == W * H and blended == (W - 1) * H and (d["taps"][:, W - 1] == 1).all()
    assert _bits_equal(out[:, W - 1], fr[:, W - 1]) and _bits_equal(tout[:, W - 1], T[:, W - 1])
    # the same in y, both ways: row 0 has iy = -1, row H - 1 has iy + 1 = H
    for dy, row in ((-0.25, 0), (0.25, H - 1)):
        rn, rh, fin_h, fin_n = _shifted(0.0, dy)
        out, _, kept, blended, d = _run(rn, rh, fr, fin_h, fin_n)
        assert kept == W * H and blended == W * (H - 1) and (d["taps"][row] == 1).all() and _bits_equal(out[row], fr[row]), dy
    # a pixel and a quarter: the far column projects outside and restarts (step 4), the next one has one tap
    rn, rh, fin_h, fin_n = _shifted(-1.25)
    out, _, kept, blended, d = _run(rn, rh, fr, fin_h, fin_n)
    assert not out[:, W - 1].any() and kept == (W - 1) * H and blended == (W - 2) * H and _bits_equal(out[:, W - 2], fr[:, W - 1])


def test_snap_on_either_side():
    fr = _frame(count=8.0)
    for dx in (0.01, -0.01):                                    # wx = 0.99 snaps up to the next pixel, wx = 0.01 snaps down: the identity either way
        rn, rh, fin_h, fin_n = _shifted(dx, dx)
        out, _, kept, blended, d = _run(rn, rh, fr, fin_h, fin_n)
        assert kept == W * H and blended == 0 and _bits_equal(out, fr), dx
        out, _, kept, blended, d = _run(rn, rh, fr, fin_h, fin_n, snap=0.0)
        assert kept == W * H and blended >= (W - 1) * (H - 1) and not _bits_equal(out, fr), dx
        assert np.abs(_mean(out)[1:-1, 1:-1] - _mean(fr)[1:-1, 1:-1]).max() < 0.05
    rn, rh, fin_h, fin_n = _shifted(0.1)                        # beyond the default snap, within a snap of 0.2
    assert _run(rn, rh, fr, fin_h, fin_n)[3] == (W - 1) * H and _run(rn, rh, fr, fin_h, fin_n, snap=0.2)[3] == 0


def test_bad_pixels_of_frame_and_t():
    rn, rh, fin_h, fin_n = _shifted(0.5)                        # new (px, py) blends old px - 1 and px
    fr = _frame(count=8.0)
    T = _moments(fr, 8.0)
    fr[1, 1, 0] = np.nan
    fr[1, 3, 2] = np.inf
    fr[2, 2] = (1.0, 1.0, 1.0, 0.0)
    fr[3, 4] = (1.0, 1.0, 1.0, -2.0)
    fr[4, 5, 3] = np.nan
    T[0, 2, 2] = 0.0
    T[0, 4, 2] = -1.0
    T[0, 6, 0] = np.nan
    T[5, 2, 1] = np.inf
    T[5, 3, 2] = np.nan                                         # (5, 3) and (5, 2): both taps of new (5, 3) are out of T's blend
    out, tout, kept, blended, d = _run(rn, rh, fr, fin_h, fin_n, T)
    assert kept == W * H
    for y, x in ((1, 1), (1, 3), (2, 2), (3, 4), (4, 5)):      # the bad old pixel is no tap: its two new pixels copy their other tap
        assert d["taps"][y, x] == 1 and d["taps"][y, x + 1] == 1
        assert _bits_equal(out[y, x], fr[y, x - 1]) and _bits_equal(out[y, x + 1], fr[y, x + 1]), (y, x)
        assert _bits_equal(tout[y, x], T[y, x - 1]) and _bits_equal(tout[y, x + 1], T[y, x + 1]), (y, x)
    assert blended == (W - 1) * H - 10
    for y, x in ((0, 2), (0, 4), (0, 6), (5, 2)):               # FRAME still blends both; T takes the good tap alone, at weight 1
        for nx, good in ((x, x - 1), (x + 1, x + 1)):
            if (y, nx) == (5, 3):
                continue
            assert d["taps"][y, nx] == 2 and np.isfinite(out[y, nx]).all()
            assert np.abs(tout[y, nx, :3] - T[y, good, :3]).max() < 1e-5 and tout[y, nx, 3] == 0, (y, nx)
    assert d["taps"][5, 3] == 2 and not tout[5, 3].any() and out[5, 3, 3] == 8.0
    assert np.isfinite(out).all() and np.isfinite(tout).all()
    # non-finite feature records of the new pixel restart it
    rn2 = rn.copy()
    rn2[4, 5, 0] = np.nan
    rn2[4, 6, 2] = np.inf
    out, _, kept, _, _ = _run(rn2, rh, _frame(count=8.0), fin_h, fin_n)
    assert kept == W * H - 2 and not out[4, 5].any() and not out[4, 6].any()


def test_overlay_pixels_restart():
    rn, rh, fin_h, fin_n = _shifted(0.5, mouse=(4.0, 2.0, 0.0))
    assert overlay(W, H, fin_n).sum() == 1 and overlay(W, H, fin_n)[2, 4]
    fr = _frame(count=8.0)
    T = _moments(fr, 8.0)
    out, tout, kept, blended, _ = _run(rn, rh, fr, fin_h, fin_n, T)
    assert kept == W * H - 1 and blended == (W - 1) * H - 1 and not out[2, 4].any() and not tout[2, 4].any()
    base = _run(rn, rh, fr, fin_h, _fin(origin=(0.5, 0.0, 0.0)), T)
    m = np.ones((H, W), bool)
    m[2, 4] = False
    assert _bits_equal(out[m], base[0][m]) and _bits_equal(tout[m], base[1][m])


def test_history_cap_on_a_blended_count():
    rn, rh, fin_h, fin_n = _shifted(0.5)
    fr = _frame(count=100.0)
    fr[:, 3, :] *= f32(0.04)                                    # column 3: count 4; new column 3 blends 100 and 4 to 52, column 4 likewise
    T = _moments(fr, 50.0)
    out, tout, kept, blended, _ = _run(rn, rh, fr, fin_h, fin_n, T, mh=10.0)
    assert kept == W * H and (out[..., 3] == 10.0).all() and (tout[..., 2] == 10.0).all()
    m = _mean(fr)
    assert np.abs(_mean(out)[:, 1:] - 0.5 * (m[:, :-1] + m[:, 1:])).max() < 1e-4
    out, tout, _, _, _ = _run(rn, rh, fr, fin_h, fin_n, T, mh=64.0)
    assert np.abs(out[:, 3:5, 3] - 52.0).max() < 1e-3 and (out[:, 1:3, 3] == 64.0).all() and (out[:, 0, 3] == 64.0).all()
    assert np.abs(tout[:, 1:, 2] - 50.0).max() < 1e-3
    assert np.abs(_mean(out)[:, 1:] - 0.5 * (m[:, :-1] + m[:, 1:])).max() < 1e-4


def test_view_dependent_materials_and_the_flag():
    fin_h, fin_n = _fin(), _fin(origin=(0.5, 0.0, 0.0))
    rh, rn = _records(fin_h, miss_cols=(0, 1)), _records(fin_n, miss_cols=(0, 1))
    fr = _frame(count=8.0)
    out, _, kept, blended, _ = _run(rn, rh, fr, fin_h, fin_n, vd=(1,))
    # the misses stay: points at infinity, which a translation leaves where they were
    assert kept == 2 * H and blended == 0 and not out[:, 2:].any() and _bits_equal(out[:, :2], fr[:, :2])
    out, _, kept, blended, d = _run(rn, rh, fr, fin_h, fin_n, vd=(1,), allm=True)
    assert kept == W * H and blended == (W - 3) * H           # column 2: a hit whose left tap is a miss
    assert (d["taps"][:, 2] == 1).all() and _bits_equal(out[:, 2], fr[:, 2])


def test_kept_set_contains_the_nearest_models():
    for seed in (1, 2, 3, 4):
        rn, rh, fr, T, fin_h, fin_n, _, _ = _random_case(seed)
        vd, M = np.array([0], np.uint8), cam_rot(fin_h["rotation"])
        for floor in (0.0, 0.2):
            near = reproject(rn, rh, fr, T, fin_h, fin_n, vd, M, 64.0, 0.05, 0.5)
            out, tout, kept, blended, d = reproject_bilinear(rn, rh, fr, T, fin_h, fin_n, vd, M, 64.0, 0.05, 0.5, SNAP, False, floor, detail=True)
            assert 0 < near[2] <= kept < W * H and 0 < blended <= kept
            assert (out[..., 3] > 0)[near[0][..., 3] > 0].all()
            assert kept == int((d["taps"] >= 1).sum()) == int((out[..., 3] > 0).sum()) and blended == int((d["taps"] >= 2).sum())
            assert not out[d["taps"] == 0].any() and not tout[d["taps"] == 0].any()


# ---------------------------------------------------------------------------------------------------------------- the oracle experiment

def _clamped_rmse(frame, ref, where):
    with np.errstate(all="ignore"):
        img = frame[..., :3] / np.maximum(frame[..., 3:4], f32(1e-30))
    img = np.where(frame[..., 3:4] > 0, img, 0)
    ok = where & np.isfinite(img).all(-1) & np.isfinite(ref).all(-1)
    d = np.clip(img[ok], 0, 1).astype(np.float64) - np.clip(ref[ok], 0, 1)
    return float(np.sqrt((d ** 2).mean()))


def test_bilinear_beats_nearest_under_a_slow_camera_move_on_m1(pt, oracle):
    """M1 in its rest pose without its texture at 128 x 72, the oracle's frames and the models: 4 frames, then 16 steps of (ORIGIN moves by
    (0.011, 0, 0.017), reproject (64, 0.02, 0.9), 4 frames), with pt_reproject_frame's model and with this one (snap 1/64) on the same frames;
    RMSE of the clamped means against a 128-frame reference of the last pose, over the whole image and over the decile of pixels with the
    steepest reference luminance gradient.  Measured with these models (deterministic) at the last step: whole image nearest 0.0773, bilinear
    0.0475, reset-and-render 0.1501; edge decile nearest 0.1814, bilinear 0.1136; kept per step nearest 9013 .. 9111 of 9216 (97.8 - 98.9 %),
    bilinear 9160 .. 9205 (99.4 - 99.9 %), of which 8965 .. 9041 blended; the median distance of the projected point from a pixel centre is
    0.38 pixel.  The last step's two comparisons are asserted; every step's figures are printed, the earlier ones against an 8-frame reference
    of their own pose, whose noise both calls share."""
    w, h, k, steps = 128, 72, 4, 16
    seed = pt.scenes.frame_seed
    base = pt.scenes.m1_moving(0, w, h, textured=False)
    vd = material_flags(base.buffers[14])
    assert not vd.any()
    M = cam_rot(base.buffers[1])

    def pose(i):
        wl = pt.scenes.m1_moving(0, w, h, textured=False)
        org = np.asarray(wl.buffers[0], f32).copy()
        org[:3] = (np.asarray(base.buffers[0], f32)[:3] + f32(i) * np.array([0.011, 0.0, 0.017], f32)).astype(f32)
        wl.buffers[0] = org
        fin = {"params": wl.buffers[4], "origin": org, "rotation": wl.buffers[1], "mouse": wl.buffers[2]}
        return oracle.Scene.from_workload(wl), _cpu_features(oracle, wl), fin

    def add(frame, T, fresh):
        return (frame + fresh[0]).astype(f32), (T + fresh[1]).astype(f32)

    sc, feat, fin = pose(0)
    zero = np.zeros((h, w, 4), f32)
    first = _accumulate(oracle, sc, w, h, [seed(f) for f in range(2, 2 + k)])
    near = bil = add(zero, zero, first)
    ref_seeds = [seed(f) for f in range(5001, 5129)]
    every = np.ones((h, w), bool)
    offs = []
    for i in range(1, steps + 1):
        sc_n, feat_n, fin_n = pose(i)
        fresh = _accumulate(oracle, sc_n, w, h, [seed(f) for f in range(2 + k * i, 2 + k * i + k)])
        a = reproject(feat_n, feat, near[0], near[1], fin, fin_n, vd, M, 64.0, 0.02, 0.9)
        b = reproject_bilinear(feat_n, feat, bil[0], bil[1], fin, fin_n, vd, M, 64.0, 0.02, 0.9, SNAP, detail=True)
        near, bil = add(a[0], a[1], fresh), add(b[0], b[1], fresh)
        on = b[4]["taps"] > 0
        off = np.hypot((b[4]["sx"] - np.floor(b[4]["sx"]) - 0.5)[on], (b[4]["sy"] - np.floor(b[4]["sy"]) - 0.5)[on])
        offs.append(float(np.median(off)))
        ref, _ = _accumulate(oracle, sc_n, w, h, ref_seeds if i == steps else ref_seeds[:8])
        ref = ref[..., :3] / ref[..., 3:4]
        Y = (0.2126 * ref[..., 0] + 0.7152 * ref[..., 1] + 0.0722 * ref[..., 2]).astype(np.float64)
        gy, gx = np.gradient(np.clip(Y, 0, 1))
        g = np.hypot(gx, gy)
        edge = g >= np.quantile(g, 0.9)
        e_near, e_bil, e_reset = (_clamped_rmse(f, ref, every) for f in (near[0], bil[0], fresh[0]))
        d_near, d_bil = _clamped_rmse(near[0], ref, edge), _clamped_rmse(bil[0], ref, edge)
        print(f"M1 {w}x{h} step {i}: kept nearest {a[2]} bilinear {b[2]} (blended {b[3]}) of {w * h}; clamped RMSE nearest {e_near:.4f} bilinear {e_bil:.4f} "
              f"reset-and-render {e_reset:.4f}; edge decile nearest {d_near:.4f} bilinear {d_bil:.4f}; median offset {offs[-1]:.2f} px")
        assert b[2] >= a[2]
        sc, feat, fin = sc_n, feat_n, fin_n
    assert e_bil < e_near, (e_bil, e_near)
    assert d_bil < d_near, (d_bil, d_near)
