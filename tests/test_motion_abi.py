"""CPU: reprojection across moved geometry (include/pt_motion.h) — exported symbols, a strict-C99 client, hand cases of the float32 model
(tests/_motion_model.py) that tests/test_gpu_motion.py holds the device to, and the oracle experiment the surface rests on."""
import ctypes
import glob
import os
import subprocess

import numpy as np

import _motion_model as MM
from _demod_model import reproject_demod
from _reproject_model import cam_rot, material_flags, reproject
from test_adaptive_abi import _declared
from test_fill_abi import _accumulate, _bits_equal, _cpu_features
from test_reproject_abi import H, W, _fin, _frame, _records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAMES = ["pt_motion_mark", "pt_reproject_frame_moved"]


def test_hip_library_exports_the_motion_symbols(pt):
    from pathtracer_0_amd import build
    lib = ctypes.CDLL(build.build_hip())
    assert _declared("pt_motion.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), n
    others = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h")) if os.path.basename(p) != "pt_motion.h")
    assert "pt_reproject.h" in others and "pt_api.h" in others
    for other in others:
        assert not set(NAMES) & set(_declared(other)), other


def test_motion_header_compiles_as_c99(tmp_path):
    src = tmp_path / "client.c"
    src.write_text('#include "pt_api.h"\n#include "pt_motion.h"\n#include <stddef.h>\n'
                   "int main(void) {\n"
                   "    int64_t kept = 0;\n"
                   "    int (*m)(pt_ctx*) = pt_motion_mark;\n"
                   "    int (*f)(pt_ctx*, float, float, float, int, float, int64_t*) = pt_reproject_frame_moved;\n"
                   "    return (m == NULL) + (f == NULL) + (int)kept + (PT_REPROJECT_ALL_MATERIALS != 1);\n}\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "client.o")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr


# ---------------------------------------------------------------------------------------------------------------- hand cases of the model

NO_EL = np.zeros((0, 10), f32)
# one triangle in the plane z = 4 that covers the 8 x 6 view of _records (hit code 0x1000000), and the same moved one pixel (1.0 there) along +x
BIG = np.array([[-40.0, -30.0, 4.0, 40.0, -30.0, 4.0, 0.0, 50.0, 4.0]], f32)


def _run(rn, rh, fr, fin_h, fin_n, tri_now, tri_then, el_now=NO_EL, el_then=NO_EL, T=None, vd=(0,), floor=0.0):
    return MM.reproject_moved(rn, rh, fr, T, fin_h, fin_n, np.array(vd, np.uint8), cam_rot(fin_h["rotation"]), tri_now, tri_then, el_now, el_then,
                              64.0, 0.02, 0.9, False, floor)


def test_translated_triangle_under_a_fixed_camera():
    """(i) the triangle moves by d = (1, 0, 0), one pixel on the plane z = 4: the surface point under new pixel x was at P - d, which the fixed camera
    saw one pixel further along (world +x is image -x, frag.glsl:894).  The source is the pixel the point projected to before."""
    fin = _fin()
    rec = _records(fin)
    fr = _frame()
    now = BIG.copy()
    now[0, [0, 3, 6]] += f32(1.0)
    out, _, kept = _run(rec, rec, fr, fin, fin, now, BIG)
    assert np.array_equal(out[:, :-1], fr[:, 1:]) and not out[:, -1].any() and kept == (W - 1) * H
    # and the source pixel by projecting P - d with the camera by hand
    Pp, Nt, rej, kind = MM.moved_point(rec, fin["origin"], now, BIG, NO_EL, NO_EL)
    assert (kind == 2).all() and not rej.any() and _bits_equal(Nt, rec.reshape(-1, 16)[:, 1:4])
    P = rec[..., 0:1] * rec[..., 8:11]
    assert np.allclose(Pp.reshape(H, W, 3), P - np.array([1.0, 0.0, 0.0], f32), atol=1e-5)
    sx = (1.0 - (Pp[:, 0] / Pp[:, 2])) * 0.5 * W
    xs = np.tile(np.arange(W), H)
    assert np.array_equal(np.floor(sx).astype(int), xs + 1)
    # moved the other way, with T carried
    T = np.concatenate([fr[..., :2], np.full((H, W, 1), 3.0, f32), np.zeros((H, W, 1), f32)], -1)
    out, tout, kept = _run(rec, rec, fr, fin, fin, BIG, now, T=T)
    assert np.array_equal(out[:, 1:], fr[:, :-1]) and np.array_equal(tout[:, 1:], T[:, :-1]) and not out[:, 0].any() and not tout[:, 0].any()


def test_rotated_triangle_turns_the_normal_back():
    """(ii) a triangle with a smooth normal turned by 90 degrees about z, (x, y, z) -> (-y, x, z): N~ is the normal before the turn to 1e-6 and P'
    the point before the turn"""
    then = np.array([[0.5, 0.25, 3.0, 2.5, 0.5, 3.5, 1.0, 2.0, 4.0]], f32)
    R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    now = (then.reshape(3, 3).astype(np.float64) @ R.T).astype(f32).reshape(1, 9)
    n_then = np.array([0.3, -0.5, -0.8])
    n_then /= np.linalg.norm(n_then)
    bary = np.array([0.2, 0.5, 0.3])
    p_then = bary @ then.reshape(3, 3).astype(np.float64)
    p_now, n_now = R @ p_then, R @ n_then
    rec = np.zeros((1, 16), f32)
    t = np.linalg.norm(p_now)
    rec[0, 0], rec[0, 1:4], rec[0, 8:11] = t, n_now, p_now / t
    rec[0, 7] = np.array([0x1000000], np.int32).view(f32)[0]
    Pp, Nt, rej, kind = MM.moved_point(rec, (0.0, 0.0, 0.0), now, then, NO_EL, NO_EL)
    assert kind[0] == 2 and not rej[0]
    assert np.abs(Nt[0] - n_then).max() < 1e-6 and np.abs(Pp[0] - p_then).max() < 1e-5
    assert abs(float(np.linalg.norm(Nt[0].astype(np.float64))) - 1) < 1e-6


def _random_case(seed):
    rs = np.random.RandomState(seed)
    fin_h, fin_n = _fin(), _fin(origin=(0.3, -0.1, 0.2), rotation=(0.0, 0.0, 0.0), mouse=(4.0, 2.0, 0.0))
    rh, rn = _records(fin_h, miss_cols=(0,)), _records(fin_n, miss_cols=(7,))
    code = rs.randint(0, 5, (H, W)) + np.where(rs.rand(H, W) < 0.3, 3 * 0x1000000, 0x1000000)
    hit = np.ascontiguousarray(rn[..., 7]).view(np.int32) != -1
    rn[..., 7] = np.where(hit, code, -1).astype(np.int32).view(f32)
    rn[..., 4:7] = rs.rand(H, W, 3)
    rh[..., 4:7] = rs.rand(H, W, 3)
    rn[..., 1:4] += rs.randn(H, W, 3).astype(f32) * f32(0.05)
    fr = _frame(count=100.0, seed=seed)
    fr[1, 1, 0], fr[2, 2, 3] = np.nan, 0.0
    T = rs.rand(H, W, 4).astype(f32) * f32(90)
    tri = rs.randn(5, 9).astype(f32)
    el = np.abs(rs.randn(5, 10)).astype(f32) + f32(0.1)
    return rn, rh, fr, T, fin_h, fin_n, tri, el


def test_nothing_moved_is_the_parent_model_bit_for_bit():
    """(iii) random records on five triangles and five ellipsoids (rotated ones among them) that stay where they were"""
    for seed in (1, 2, 3):
        rn, rh, fr, T, fin_h, fin_n, tri, el = _random_case(seed)
        vd, M = np.array([0], np.uint8), cam_rot(fin_h["rotation"])
        want = reproject(rn, rh, fr, T, fin_h, fin_n, vd, M, 64.0, 0.05, 0.5)
        got = _run_all(rn, rh, fr, T, fin_h, fin_n, vd, M, tri, el, 0.0)
        assert 0 < want[2] < W * H and got[2] == want[2] and _bits_equal(got[0], want[0]) and _bits_equal(got[1], want[1])
        want = reproject_demod(rn, rh, fr, T, fin_h, fin_n, vd, M, 64.0, 0.05, 0.5, False, 0.2)
        got = _run_all(rn, rh, fr, T, fin_h, fin_n, vd, M, tri, el, 0.2)
        assert got[2] == want[2] and _bits_equal(got[0], want[0]) and _bits_equal(got[1], want[1])
        _, _, rej, kind = MM.moved_point(rn, fin_n["origin"], tri, tri.copy(), el, el.copy())
        assert not rej.any() and set(np.unique(kind)) <= {0, 1}


def _run_all(rn, rh, fr, T, fin_h, fin_n, vd, M, tri, el, floor):
    return MM.reproject_moved(rn, rh, fr, T, fin_h, fin_n, vd, M, tri, tri.copy(), el, el.copy(), 64.0, 0.05, 0.5, False, floor)


def _el_record(p, n, k=0):
    rec = np.zeros((1, 16), f32)
    t = np.linalg.norm(p)
    rec[0, 0], rec[0, 1:4], rec[0, 8:11] = t, n, np.asarray(p) / t
    rec[0, 7] = np.array([3 * 0x1000000 + k], np.int32).view(f32)[0]
    return rec


def test_ellipsoid_translated_with_r_doubled():
    """(iv) a point keeps its place on the unit sphere: u = P - c shrinks by r' / r (and by sqrt(stretch / stretch') per axis)"""
    then = np.array([[1.0, 2.0, 5.0, 1.0, 4.0, 1.0, 0.0, 0.0, 0.0, 0.5]], f32)
    now = np.array([[1.5, 2.25, 6.0, 1.0, 4.0, 1.0, 0.0, 0.0, 0.0, 1.0]], f32)
    u = np.array([0.6, 0.0, -0.8])
    n = np.array([0.6, 0.0, -0.8], f32)
    Pp, Nt, rej, kind = MM.moved_point(_el_record(now[0, :3] + u * 1.0, n), (0.0, 0.0, 0.0), np.zeros((0, 9), f32), np.zeros((0, 9), f32), now, then)
    assert kind[0] == 3 and not rej[0] and _bits_equal(Nt[0], n)
    assert np.abs(Pp[0] - (then[0, :3] + u * 0.5)).max() < 1e-5
    # a stretch that changes: axis i scales by sqrt(stretch_i / stretch'_i)
    now2 = now.copy()
    now2[0, 3:6] = (4.0, 4.0, 1.0)
    Pp, _, rej, _ = MM.moved_point(_el_record(now2[0, :3] + u, n), (0.0, 0.0, 0.0), np.zeros((0, 9), f32), np.zeros((0, 9), f32), now2, then)
    assert not rej[0] and np.abs(Pp[0] - (then[0, :3] + u * 0.5 * np.array([2.0, 1.0, 1.0]))).max() < 1e-5


def test_rejections():
    """(v) a degenerate triangle (den = 0), an id beyond either count, a moved ellipsoid with a rotation, a NaN vertex, an unknown type"""
    fin = _fin()
    rec = _records(fin)
    fr = _frame()
    moved = BIG.copy()
    moved[0, [0, 3, 6]] += f32(1.0)
    assert _run(rec, rec, fr, fin, fin, moved, BIG)[2] == (W - 1) * H
    flat = moved.copy()
    flat[0, 6:9] = flat[0, 3:6]                                         # C = B: e1 = e2, den = 0
    assert _run(rec, rec, fr, fin, fin, flat, BIG)[2] == 0
    nan = moved.copy()
    nan[0, 4] = np.nan
    assert _run(rec, rec, fr, fin, fin, nan, BIG)[2] == 0
    nan_then = BIG.copy()
    nan_then[0, 0] = np.nan
    assert _run(rec, rec, fr, fin, fin, moved, nan_then)[2] == 0
    none = np.zeros((0, 9), f32)
    assert _run(rec, rec, fr, fin, fin, BIG, none)[2] == 0 and _run(rec, rec, fr, fin, fin, none, BIG)[2] == 0      # id 0 beyond one count
    assert _run(rec, rec, fr, fin, fin, BIG, BIG)[2] == W * H
    # ellipsoids
    then = np.array([[1.0, 2.0, 5.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.5]], f32)
    now = then.copy()
    now[0, 0] += f32(0.25)
    p, n = now[0, :3] + np.array([0.0, 0.0, -0.5]), np.array([0.0, 0.0, -1.0], f32)
    args = (np.zeros((0, 9), f32), np.zeros((0, 9), f32))
    assert not MM.moved_point(_el_record(p, n), (0, 0, 0), *args, now, then)[2][0]
    for rot_in in (now, then):
        a, b = now.copy(), then.copy()
        (a if rot_in is now else b)[0, 7] = f32(0.3)
        assert MM.moved_point(_el_record(p, n), (0, 0, 0), *args, a, b)[2][0]
    rot_still = then.copy()
    rot_still[0, 7] = f32(0.3)
    assert not MM.moved_point(_el_record(p, n), (0, 0, 0), *args, rot_still, rot_still.copy())[2][0]      # unmoved: a rotation is fine
    assert MM.moved_point(_el_record(p, n, k=1), (0, 0, 0), *args, now, then)[2][0]                       # id beyond the counts
    assert MM.moved_point(_el_record(p, n), (0, 0, 0), *args, now, NO_EL)[2][0]
    other = _el_record(p, n)
    other[0, 7] = np.array([2 * 0x1000000], np.int32).view(f32)[0]                                         # no such type
    assert MM.moved_point(other, (0, 0, 0), *args, now, then)[2][0]


# ---------------------------------------------------------------------------------------------------------------- the oracle experiment

def _clamped_rmse(frame, ref, where):
    img = frame[..., :3] / np.maximum(frame[..., 3:4], f32(1e-30))
    img = np.where(frame[..., 3:4] > 0, img, 0)
    ok = where & np.isfinite(img).all(-1) & np.isfinite(ref).all(-1)
    d = np.clip(img[ok], 0, 1).astype(np.float64) - np.clip(ref[ok], 0, 1)
    return float(np.sqrt((d ** 2).mean()))


def test_mark_reproject_render_beats_reset_render_on_m1(pt, oracle):
    """M1 (diffuse, no texture) at 160 x 90 with the oracle's frames and the models: 4 frames in the rest pose, then 8 steps of
    mark - move - reproject (64, 0.02, 0.9) - 4 frames, against a reset and 4 frames in the last pose; both against a 256-frame reference of the
    last pose, display-referred (RMSE of the clamped means).  Measured with these models (deterministic) at the last step: whole image 0.0575
    against 0.1422 (kept 0.996 of the pixels); over the pixels on a moved primitive, then or now (1483): 0.0980 against 0.1863.
    The figures of every step (against a 64-frame reference of that step's pose) are printed, not asserted."""
    w, h, k, steps = 160, 90, 4, 8
    seed = pt.scenes.frame_seed

    def pose(i):
        wl = pt.scenes.m1_moving(i, w, h, textured=False)
        return wl, oracle.Scene.from_workload(wl), _cpu_features(oracle, wl)

    def add(frame, T, sc, first):
        a, b = _accumulate(oracle, sc, w, h, [seed(f) for f in range(first, first + k)])
        return (frame + a).astype(f32), (T + b).astype(f32)

    wl, sc, feat = pose(0)
    fin = {"params": wl.buffers[4], "origin": wl.buffers[0], "rotation": wl.buffers[1], "mouse": wl.buffers[2]}
    M = cam_rot(fin["rotation"])
    vd = material_flags(wl.buffers[14])
    assert not vd.any()
    frame, T = add(np.zeros((h, w, 4), f32), np.zeros((h, w, 4), f32), sc, 2)
    ref_seeds = [seed(f) for f in range(5001, 5257)]
    for i in range(1, steps + 1):
        wl_n, sc_n, feat_n = pose(i)
        geo = (MM.tri_vertices(wl_n.buffers[3]), MM.tri_vertices(wl.buffers[3]), MM.ellipsoids(wl_n.buffers[7]), MM.ellipsoids(wl.buffers[7]))
        frame, T, kept = MM.reproject_moved(feat_n, feat, frame, T, fin, fin, vd, M, *geo, 64.0, 0.02, 0.9)
        frame, T = add(frame, T, sc_n, 2 + k * i)
        kind_n = MM.moved_point(feat_n, fin["origin"], *geo)[3].reshape(h, w)
        kind_h = MM.moved_point(feat, fin["origin"], geo[1], geo[0], geo[3], geo[2])[3].reshape(h, w)
        on_moved = (kind_n >= 2) | (kind_h >= 2)
        line = f"M1 {w}x{h} step {i}: kept {kept / (w * h):.3f}, on moved primitives {int(on_moved.sum())} pixels"
        ref, _ = _accumulate(oracle, sc_n, w, h, ref_seeds if i == steps else ref_seeds[:64])      # a reference of its own per step
        ref = ref[..., :3] / ref[..., 3:4]
        reset, _ = add(np.zeros((h, w, 4), f32), np.zeros((h, w, 4), f32), sc_n, 2 + k * i)
        every = np.ones((h, w), bool)
        a_all, b_all = _clamped_rmse(frame, ref, every), _clamped_rmse(reset, ref, every)
        a_mv, b_mv = _clamped_rmse(frame, ref, on_moved), _clamped_rmse(reset, ref, on_moved)
        line += f"; clamped RMSE mark-reproject-render {a_all:.4f} against reset-render {b_all:.4f}; on moved primitives {a_mv:.4f} against {b_mv:.4f}"
        print(line)
        wl, feat = wl_n, feat_n
    assert 0 < kept < w * h
    assert a_all < b_all, (a_all, b_all)
