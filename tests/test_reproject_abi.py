"""CPU: the reprojection surface (include/pt_reproject.h) — exported symbols, a strict-C99 client, and hand-computed cases of the float32 model of
the mapping (tests/_reproject_model.py) that tests/test_gpu_reproject.py holds the device to."""
import ctypes
import os
import subprocess

import numpy as np

from _reproject_model import cam_rot, frame_in, material_flags, overlay, reproject
from test_adaptive_abi import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 8, 6


def test_hip_library_exports_the_reproject_symbols(pt):
    from pathtracer_0_amd import build
    lib = ctypes.CDLL(build.build_hip())
    names = _declared("pt_reproject.h")
    assert names == ["pt_reproject_frame"]
    for n in names:
        assert hasattr(lib, n), n
    for other in ("pt_api.h", "pt_adaptive.h", "pt_denoise.h", "pt_debug.h"):
        assert not set(names) & set(_declared(other)), other


def test_reproject_header_compiles_as_c99(tmp_path):
    src = tmp_path / "client.c"
    src.write_text('#include "pt_api.h"\n#include "pt_reproject.h"\n#include <stddef.h>\n'
                   "int main(void) {\n"
                   "    int64_t kept = 0;\n"
                   "    int (*f)(pt_ctx*, float, float, float, int, int64_t*) = pt_reproject_frame;\n"
                   "    return (f == NULL) + (int)kept + (PT_REPROJECT_ALL_MATERIALS != 1);\n}\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "client.o")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr


def _fin(origin=(0.0, 0.0, 0.0), rotation=(0.0, 0.0, 0.0), mouse=(-1.0e6, -1.0e6, 0.0)):
    # screenSize 1, focalLength 1, resolution W, screenHratio H/W, BLUR 0, AUTO_FOCUS 0, FOCAL_DISTANCE 1
    return frame_in([1.0, 1.0, W, H / W, 8, 8, 0, 0.0, 1.0, 1.0, 0.0, 0.0], origin, rotation, mouse)


def _records(fin, z=4.0, miss_cols=()):
    """feature records of the camera rays of an unrotated camera facing the plane z = `z` (normal (0, 0, -1), material 0, hit code 0x1000000);
    the columns in miss_cols see the sky instead"""
    ss, fl, hr = (float(fin["params"][k]) for k in (0, 1, 3))
    rec = np.zeros((H, W, 16), np.float32)
    for py in range(H):
        for px in range(W):
            q = np.array([-((px + 0.5) / W * 2 - 1) * ss, ((py + 0.5) / H * 2 - 1) * hr * ss, fl])
            d = q / np.linalg.norm(q)
            rec[py, px, 8:11] = d
            if px in miss_cols:
                rec[py, px, 0] = -1.0
                rec[py, px, 7] = np.array([-1], np.int32).view(np.float32)[0]
                rec[py, px, 11] = np.array([-1], np.int32).view(np.float32)[0]
            else:
                t = (z - float(fin["origin"][2])) / d[2]
                rec[py, px, 0] = t
                rec[py, px, 1:4] = (0.0, 0.0, -1.0)
                rec[py, px, 7] = np.array([0x1000000], np.int32).view(np.float32)[0]
                rec[py, px, 11] = np.array([0], np.int32).view(np.float32)[0]
    return rec


def _frame(count=4.0, seed=0):
    rs = np.random.RandomState(seed)
    fr = np.concatenate([rs.rand(H, W, 3).astype(np.float32) * np.float32(count), np.full((H, W, 1), count, np.float32)], -1)
    return fr


def _run(rn, rh, fr, fin_h, fin_n, T=None, vd=(0,), mh=64.0, dt=0.02, nt=0.9, allm=False):
    return reproject(rn, rh, fr, T, fin_h, fin_n, np.array(vd, np.uint8), cam_rot(fin_h["rotation"]), mh, dt, nt, allm)


def test_identity_camera_keeps_every_pixel():
    fin = _fin()
    rec = _records(fin)
    fr = _frame()
    T = np.concatenate([fr[..., :2], np.full((H, W, 1), 3.0, np.float32), np.zeros((H, W, 1), np.float32)], -1)
    out, tout, kept = _run(rec, rec, fr, fin, fin, T)
    assert kept == W * H
    assert np.array_equal(out, fr) and np.array_equal(tout, T)


def test_translation_facing_a_plane_shifts_by_whole_pixels():
    """one pixel on the plane z = 4 is 2*screenSize/W * z / focalLength = 1.0 wide: a move of +1 in x makes new pixel x the old x - 1"""
    fin_h, fin_n = _fin(), _fin(origin=(1.0, 0.0, 0.0))
    rh, rn = _records(fin_h), _records(fin_n)
    fr = _frame()
    out, _, kept = _run(rn, rh, fr, fin_h, fin_n)
    assert np.array_equal(out[:, 1:], fr[:, :-1])
    assert not out[:, 0].any()                                  # seen from the old camera outside the image: disoccluded
    assert kept == (W - 1) * H
    # the other way round, and a move along the view axis keeps the centre
    out2, _, _ = _run(rh, rn, fr, fin_n, fin_h)
    assert np.array_equal(out2[:, :-1], fr[:, 1:]) and not out2[:, -1].any()


def test_depth_and_normal_tolerances_reject():
    fin_h, fin_n = _fin(), _fin(origin=(1.0, 0.0, 0.0))
    rh, rn = _records(fin_h), _records(fin_n)
    fr = _frame()
    rh_far = rh.copy()
    rh_far[..., 0] *= np.float32(1.1)                           # the old surface 10 % further away
    assert _run(rn, rh_far, fr, fin_h, fin_n, dt=0.02)[2] == 0
    assert _run(rn, rh_far, fr, fin_h, fin_n, dt=0.2)[2] == (W - 1) * H
    rh_tilt = rh.copy()
    rh_tilt[..., 1:4] = (0.0, -0.6, -0.8)                       # dot = 0.8
    assert _run(rn, rh_tilt, fr, fin_h, fin_n, nt=0.9)[2] == 0
    assert _run(rn, rh_tilt, fr, fin_h, fin_n, nt=0.7)[2] == (W - 1) * H
    rh_mat = rh.copy()
    rh_mat[..., 11] = np.array([1], np.int32).view(np.float32)[0]      # another material
    assert _run(rn, rh_mat, fr, fin_h, fin_n, vd=(0, 0))[2] == 0


def test_history_cap_scales_sums():
    fin = _fin()
    rec = _records(fin)
    fr = _frame(count=100.0)
    fr[0, 0, 3] = 5.0                                           # below the cap: untouched
    T = np.zeros((H, W, 4), np.float32)
    T[..., 0], T[..., 1], T[..., 2] = 30.0, 90.0, 50.0
    out, tout, kept = _run(rec, rec, fr, fin, fin, T, mh=10.0)
    assert kept == W * H
    f = np.float32(10.0) / np.float32(100.0)
    assert np.array_equal(out[1:, :, :3], fr[1:, :, :3] * f) and (out[1:, :, 3] == 10.0).all()
    assert np.array_equal(out[0, 0], fr[0, 0])
    g = np.float32(10.0) / np.float32(50.0)
    assert (tout[..., 0] == np.float32(30.0) * g).all() and (tout[..., 1] == np.float32(90.0) * g).all() and (tout[..., 2] == 10.0).all()


def test_nan_inf_alpha0_and_overlay_pixels_restart():
    fin_h = _fin()
    fin_n = _fin(mouse=(4.0, 2.0, 0.0))                         # overlay half-width 8 * 0.005: exactly pixel (4, 2)
    assert overlay(W, H, fin_n).sum() == 1 and overlay(W, H, fin_n)[2, 4]
    rec = _records(fin_h)
    fr = _frame()
    fr[1, 1, 0] = np.nan
    fr[1, 2, 2] = np.inf
    fr[3, 3] = (1.0, 1.0, 1.0, 0.0)
    rn = rec.copy()
    rn[4, 5, 0] = np.nan                                        # t not finite
    rn[4, 6, 2] = np.inf                                        # N not finite
    out, _, kept = _run(rn, rec, fr, fin_h, fin_n)
    bad = [(1, 1), (1, 2), (3, 3), (2, 4), (4, 5), (4, 6)]
    for y, x in bad:
        assert not out[y, x].any(), (y, x)
    m = np.ones((H, W), bool)
    for y, x in bad:
        m[y, x] = False
    assert np.array_equal(out[m], fr[m]) and kept == W * H - len(bad)


def test_miss_beside_a_hit():
    fin = _fin()
    rec = _records(fin, miss_cols=(0, 1, 2))
    fr = _frame()
    out, _, kept = _run(rec, rec, fr, fin, fin)
    assert kept == W * H and np.array_equal(out, fr)            # both kinds map onto themselves
    rh = _records(fin, miss_cols=(1, 2, 3))                     # column 0: miss over a hit; column 3: hit over a miss
    out, _, kept = _run(rec, rh, fr, fin, fin)
    assert not out[:, 0].any() and not out[:, 3].any()
    assert kept == (W - 2) * H
    # a miss seen from a moved camera is a point at infinity: a translation keeps it in place
    out, _, _ = _run(_records(_fin(origin=(1.0, 0.0, 0.0)), miss_cols=range(W)), _records(fin, miss_cols=range(W)), fr, fin,
                     _fin(origin=(1.0, 0.0, 0.0)))
    assert np.array_equal(out, fr)


def test_view_dependent_materials_and_the_flag():
    fin = _fin()
    rec = _records(fin, miss_cols=(0,))
    fr = _frame()
    out, _, kept = _run(rec, rec, fr, fin, fin, vd=(1,))
    assert kept == H and np.array_equal(out[:, 0], fr[:, 0]) and not out[:, 1:].any()      # the misses stay
    out, _, kept = _run(rec, rec, fr, fin, fin, vd=(1,), allm=True)
    assert kept == W * H and np.array_equal(out, fr)


def test_material_flags_rule():
    def mat(**kw):
        F = np.zeros(48, np.float32)
        F[[22, 23, 24, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41]] = -1.0      # every map_* slot: none
        F[26] = 1.0                                             # Pr = 1: fully rough
        F[21] = 2.0                                             # illum
        F[12] = 0.0
        for k, v in kw.items():
            F[{"Tr": 12, "Tf0": 13, "illum": 21, "Pr": 26, "Pc": 28, "map_Pr": 33, "map_Pc": 35, "map_Tr": 39, "map_Kd": 23}[k]] = v
        return F
    cases = [({}, 0), ({"Pr": 0.5}, 1), ({"Pc": 0.2}, 1), ({"Tr": 0.1}, 1), ({"Tf0": 0.5}, 1), ({"illum": 5}, 1), ({"illum": 7}, 1),
             ({"map_Pr": 0}, 1), ({"map_Pc": 3}, 1), ({"map_Tr": 1}, 1), ({"map_Kd": 2}, 0), ({"Pr": np.nan}, 1)]
    recs = [mat(**kw) for kw, _ in cases]
    mtl = np.concatenate(recs).astype(np.float32)                # F[k] == mtlData[48*m + k] (buildScene): mtlData[0] = 48 overlays F[0] of record 0
    mtl[0] = 48.0
    mtl = np.concatenate([mtl, [0.0]]).astype(np.float32)
    got = material_flags(mtl)
    assert list(got) == [want for _, want in cases]
