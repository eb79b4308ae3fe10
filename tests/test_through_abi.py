"""CPU: seen-through feature records (include/pt_through.h) — exported symbols, a strict-C99 client, hand cases of the float32 model
(tests/_through_model.py) that tests/test_gpu_through.py holds the device to, and the oracle experiment the surface rests on."""
import ctypes
import os
import subprocess

import numpy as np

import _through_model as TM
from _fill_model import denoise_guided_filled, lattice
from test_adaptive_abi import _declared
from test_fill_abi import _accumulate, _bits_equal, _cpu_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
f32 = np.float32
NAMES = ["pt_denoise_guided_through", "pt_fill_frame_through", "pt_read_display_denoised_guided_through", "pt_read_features_through",
         "pt_read_through_rays"]
OTHERS = ("pt_api.h", "pt_debug.h", "pt_adaptive.h", "pt_denoise.h", "pt_reproject.h", "pt_guided.h", "pt_steer.h", "pt_demod.h", "pt_fill.h", "pt_scene.h")


def test_hip_library_exports_the_through_symbols(pt):
    from pathtracer_0_amd import build
    lib = ctypes.CDLL(build.build_hip())
    assert _declared("pt_through.h") == NAMES
    for n in NAMES:
        assert hasattr(lib, n), n
    for other in OTHERS:
        assert not set(NAMES) & set(_declared(other)), other


def test_through_header_compiles_as_c99(tmp_path):
    src = tmp_path / "client.c"
    src.write_text('#include "pt_api.h"\n#include "pt_through.h"\n#include <stddef.h>\n'
                   "int main(void) {\n"
                   "    pt_through_rule r = {4, 0.8f, PT_THROUGH_REFLECT | PT_THROUGH_TRANSMIT, PT_THROUGH_KEY};\n"
                   "    int (*a)(pt_ctx*, const pt_through_rule*, float*) = pt_read_features_through;\n"
                   "    int (*b)(pt_ctx*, const pt_through_rule*, float*) = pt_read_through_rays;\n"
                   "    int (*f)(pt_ctx*, const pt_through_rule*, float, float, float, float, float*, int64_t*) = pt_fill_frame_through;\n"
                   "    int (*d)(pt_ctx*, const pt_through_rule*, int, float, float, float, float, int, float, float*) = pt_denoise_guided_through;\n"
                   "    int (*v)(pt_ctx*, const pt_through_rule*, int, float, float, float, float, int, float, int, uint8_t*) =\n"
                   "        pt_read_display_denoised_guided_through;\n"
                   "    return (a == NULL) + (b == NULL) + (f == NULL) + (d == NULL) + (v == NULL) + (r.max_depth != 4) + (PT_THROUGH_RAY_FLOATS != 8);\n}\n")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                          "-o", str(tmp_path / "client.o")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr


# ---------------------------------------------------------------------------------------------------------------- hand cases of the model

def _mat(Kd=(0.8, 0.8, 0.8), Pm=0.0, Pr=1.0, Pc=0.0, Tr=0.0, Ni=1.0, illum=2):
    m = np.zeros(49, f32)
    m[4:7] = Kd
    m[12], m[16], m[21], m[25], m[26], m[28] = Tr, Ni, illum, Pm, Pr, Pc
    m[[22, 23, 24]] = -1
    m[32:42] = -1
    return m


def _planes(planes):
    """rayScene over infinite planes (point, normal, material), in float64 rounded: enough for the model, which only consumes the hits"""
    def ray(o, d):
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        best = None
        for i, (q, n, mat) in enumerate(planes):
            den = float(np.dot(n, d))
            if den == 0:
                continue
            t = float(np.dot(np.asarray(q, np.float64) - o, n)) / den
            if t > 1e-6 and (best is None or t < best[0]):
                best = (t, i, n, mat)
        if best is None:
            return -1, np.zeros(8, f32)
        t, i, n, mat = best
        return 0x1000000 + i, np.array([t, *(o + t * d), *n, mat], f32)
    return ray


S = np.sqrt(0.5)
MIRROR, FLOOR = _mat(Kd=(0.9, 0.8, 0.5), Pm=1.0, Pr=0.0), _mat(Kd=(0.5, 0.25, 0.75))
TILTED = ((0.0, 1.0, 2.0), (0.0, -S, -S), 0)                # a mirror at 45 degrees in front of the camera, sending +z down
GROUND = ((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1)


def _i32(x):
    return int(np.float32(x).view(np.int32))


def test_a_mirror_over_a_floor_records_the_floor():
    ray = _planes([TILTED, GROUND])
    c = TM.chain(ray, [MIRROR, FLOOR], (0, 1, 0), (0, 0, 1), 4, 0.8, TM.REFLECT, TM.KEY)
    rec = c["rec"]
    assert c["k"] == 1 and c["codes"] == [0x1000000, 0x1000001]
    t1, t2 = f32(2.0), f32(ray((0, 1, 2), (0, -1, 0))[1][0])
    assert abs(float(t2) - 1.0) < 1e-6
    assert np.isclose(rec[0], t1 + t2, rtol=1e-6, atol=0)                       # L = t1 + t2
    assert np.array_equal(rec[1:4], f32([0, 1, 0]))                            # the floor's N
    assert np.array_equal(rec[4:7], (f32(1) * MIRROR[4:7]) * FLOOR[4:7])       # Kd in chain order
    assert _i32(rec[7]) == 0x1000001
    assert np.array_equal(rec[8:11], f32([0, 0, 1]))                           # D0, not the last direction
    assert _i32(rec[11]) == (1 << 24) | (0 << 12) | 1                          # the key
    assert _i32(rec[14]) == 1
    assert np.allclose(c["ray"][:3], [0, 1, 2], atol=1e-6) and np.allclose(c["last_dir"], [0, -1, 0], atol=1e-6) and _i32(c["ray"][7]) == 1
    # without the key the word is the floor's material; a weight below min_weight, or the lobe switched off, stays on the mirror
    assert _i32(TM.chain(ray, [MIRROR, FLOOR], (0, 1, 0), (0, 0, 1), 4, 0.8, TM.REFLECT, 0)["rec"][11]) == 1
    half = _mat(Kd=(0.9, 0.8, 0.5), Pm=0.0, Pr=0.0)                            # r = 1, d = 1: r' = 0.5
    assert TM.chain(ray, [half, FLOOR], (0, 1, 0), (0, 0, 1), 4, 0.8, TM.REFLECT, TM.KEY)["k"] == 0
    assert TM.chain(ray, [half, FLOOR], (0, 1, 0), (0, 0, 1), 4, 0.5, TM.REFLECT, TM.KEY)["k"] == 1
    assert TM.chain(ray, [MIRROR, FLOOR], (0, 1, 0), (0, 0, 1), 4, 0.8, TM.TRANSMIT, TM.KEY)["k"] == 0
    assert TM.chain(ray, [MIRROR, FLOOR], (0, 1, 0), (0, 0, 1), 4, 0.8, TM.REFLECT, TM.KEY, raytracing=False)["k"] == 0
    # max_depth caps the chain: two facing mirrors
    facing = _planes([((0, 0, 2), (0, 0, -1), 0), ((0, 0, -2), (0, 0, 1), 0)])
    for depth in (0, 1, 3, 8):
        c = TM.chain(facing, [MIRROR], (0, 0, 0), (0, 0, 1), depth, 0.8, TM.REFLECT, TM.KEY)
        assert c["k"] == depth and len(c["codes"]) == depth + 1
        assert np.isclose(c["rec"][0], 2 + 4 * depth, rtol=1e-6)


def test_a_chain_that_leaves_into_the_sky_keeps_the_mirror():
    ray = _planes([((0.0, 0.0, 2.0), (0.0, 0.0, -1.0), 0)])
    c = TM.chain(ray, [MIRROR], (0, 1, 0), (0, 0, 1), 4, 0.8, TM.REFLECT, TM.KEY)
    first = TM.chain(ray, [MIRROR], (0, 1, 0), (0, 0, 1), 0, 0.8, TM.REFLECT, TM.KEY)
    assert c["k"] == 0 and c["codes"] == [0x1000000] and _bits_equal(c["rec"], first["rec"]) and _bits_equal(c["ray"], first["ray"])
    assert _i32(c["rec"][11]) == 0 and _i32(c["rec"][14]) == 0
    # and a first ray that misses has the miss record
    c = TM.chain(ray, [MIRROR], (0, 1, 0), (0, 0, -1), 4, 0.8, TM.REFLECT, TM.KEY)
    assert c["rec"][0] == -1 and _i32(c["rec"][7]) == -1 and _i32(c["rec"][11]) == -1 and not c["rec"][1:7].any() and c["ray"][3] == -1


def test_total_internal_reflection_stops_the_chain():
    """a ray enters a glass slab through a tilted face and meets the far face beyond the critical angle: fresnelReflectAmount returns 1 there, the
    transmission weight is 0, and a rule that follows transmission only stops on that face; refract itself answers such a pair with the zero vector"""
    glass = _mat(Kd=(1.0, 0.9, 0.8), Pr=1.0, Tr=0.9, Ni=1.5)
    ray = _planes([((0, 0, 1), (0, 0, -1), 0), ((0, 2, 0), (0, 1, 0), 0), ((0, 0, 10), (0, 0, -1), 0)])
    d = np.array([0.0, 0.8, 0.6])
    c = TM.chain(ray, [glass], (0, 0, 0), d, 4, 0.5, TM.TRANSMIT, TM.KEY)
    assert c["k"] == 1 and c["codes"] == [0x1000000, 0x1000001]
    assert np.array_equal(c["rec"][4:7], (f32(1) * glass[4:7]) * glass[4:7])
    both = TM.chain(ray, [glass], (0, 0, 0), d, 2, 0.5, TM.REFLECT | TM.TRANSMIT, TM.KEY)
    assert both["k"] == 2 and both["codes"][:2] == c["codes"]                 # the reflection lobe has all the weight there and is followed
    inside = c["last_dir"]
    assert all(x == 0 for x in TM.refract(list(inside), TM.v3(0, -1, 0), f32(1.5) / f32(1.0029)))
    assert not all(x == 0 for x in TM.refract(TM.v3(0, 0.8, 0.6), TM.v3(0, 0, -1), f32(1.0029) / f32(1.5)))


def test_a_direction_that_is_not_finite_or_zero_stops_at_step_seven():
    """the weights of a polished metal do not read N, so reflection is chosen (r' = 1) whatever N holds: a NaN normal (a triangle without vertex
    normals) makes reflect(D, N) NaN and the chain stops on that surface with its record written; the same for a zero vector"""
    floor = _planes([GROUND])

    def ray(o, d):                                     # a surface with a NaN normal in front of the camera, the ground below
        if o[2] < 1.5 and d[2] > 0:
            t = (2.0 - float(o[2])) / float(d[2])
            return 0x1000000, np.array([t, o[0] + t * d[0], o[1] + t * d[1], 2.0, np.nan, np.nan, np.nan, 0], f32)
        return floor(o, d)
    c = TM.chain(ray, [MIRROR, FLOOR], (0, 1, 0), (0, 0, 1), 4, 0.8, TM.REFLECT, TM.KEY)
    assert c["k"] == 0 and c["codes"] == [0x1000000] and np.isnan(c["rec"][1:4]).all() and c["rec"][0] == 2 and c["margin"] > 0.1
    e = TM.chain(ray, [MIRROR, FLOOR], (0, 1, 0), (0, 0, 1), 4, 0.8, TM.REFLECT, TM.KEY, exact_dirs=True)
    assert e["k"] == 0 and e["codes"] == c["codes"]
    # a zero vector: refract's answer where its own k < 0 although the weights let transmission through (Tr from a material whose fresnel
    # term sees n1 <= n2 by a stale stack slot): stubbed here by a refract that returns it
    glass = _mat(Kd=(1.0, 0.9, 0.8), Pr=1.0, Tr=0.9, Ni=1.5)
    slab = _planes([((0, 0, 1), (0, 0, -1), 0), ((0, 0, 3), (0, 0, -1), 0)])
    keep = TM.refract
    try:
        TM.refract = lambda I, N, eta: TM.v3(0, 0, 0)
        z = TM.chain(slab, [glass], (0, 0, 0), (0, 0, 1), 4, 0.5, TM.TRANSMIT, TM.KEY)
    finally:
        TM.refract = keep
    assert z["k"] == 0 and z["codes"] == [0x1000000]
    assert TM.chain(slab, [glass], (0, 0, 0), (0, 0, 1), 4, 0.5, TM.TRANSMIT, TM.KEY)["k"] >= 1


def test_fma_is_exactly_rounded():
    rs = np.random.RandomState(3)
    from fractions import Fraction
    for _ in range(2000):
        a, b = f32(rs.randn()), f32(rs.randn())
        c = f32(-(float(a) * float(b)) * (1 + rs.randn() * 1e-7)) if rs.rand() < 0.5 else f32(rs.randn() * 10.0 ** rs.randint(-8, 8))
        exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        lo = f32(float(exact))                                                  # float(Fraction) rounds correctly to binary64: bracket in binary32 by hand
        cands = sorted({float(lo), float(np.nextafter(lo, f32(np.inf))), float(np.nextafter(lo, f32(-np.inf)))}, key=lambda v: abs(Fraction(v) - exact))
        got = float(TM.fma(a, b, c))
        assert abs(Fraction(got) - exact) == abs(Fraction(cands[0]) - exact), (a, b, c, got, cands)


def _dirs(wl):
    from _reproject_ref64 import camera_dirs as _camera_dirs
    return _camera_dirs(wl, wl.W, wl.H).astype(f32)


def test_depth_zero_is_the_first_hit_model(pt, oracle):
    wl = pt.scenes.build("C3", 48, 27)
    want = _cpu_features(oracle, wl)
    for rule in ((0, 0.8, TM.REFLECT | TM.TRANSMIT, TM.KEY), (4, 0.5, 0, TM.KEY)):
        got, rays, _ = TM.through_features(oracle, wl, _dirs(wl), *rule)
        assert _bits_equal(got, want), rule
        assert _bits_equal(rays[..., 3], want[..., 0]) and _bits_equal(rays[..., 4:7], want[..., 8:11]) and not rays[..., 7].view(np.int32).any()
    deep, _, _ = TM.through_features(oracle, wl, _dirs(wl), 4, 0.5, TM.REFLECT | TM.TRANSMIT, TM.KEY)
    k = np.ascontiguousarray(deep[..., 14]).view(np.int32)
    assert (k > 0).any() and _bits_equal(deep[k == 0], want[k == 0])            # a pixel whose chain takes no step keeps the first-hit record


# ---------------------------------------------------------------------------------------------------------------- the oracle experiment

def _rmse(img, ref, where):
    ok = where & np.isfinite(img).all(-1) & np.isfinite(ref).all(-1)
    d = np.clip(img[ok], 0, 1).astype(np.float64) - np.clip(ref[ok], 0, 1)
    u = img[ok].astype(np.float64) - ref[ok]
    return float(np.sqrt((d ** 2).mean())), float(np.sqrt((u ** 2).mean()))


def _experiment(pt, oracle, name, w, h, rules):
    wl = pt.scenes.build(name, w, h)
    sc = oracle.Scene.from_workload(wl)
    first = _cpu_features(oracle, wl)
    seed = pt.scenes.frame_seed
    ref, _ = _accumulate(oracle, sc, w, h, [seed(f) for f in range(5001, 5129)])
    ref = ref[..., :3] / ref[..., 3:4]
    args = (5, 2.0, 0.3, 0.05, INF, 4, 0.2)
    mats = TM.materials(wl.buffers[14])
    fmat = np.ascontiguousarray(first[..., 11]).view(np.int32)
    metal = np.isin(fmat, [k for k, m in enumerate(mats) if m[25] == 1])
    glass = np.isin(fmat, [k for k, m in enumerate(mats) if m[12] > 0])
    feats = {"first-hit": first}
    for label, rule in rules.items():
        feats[label] = TM.through_features(oracle, wl, _dirs(wl), *rule)[0]
    out = {}
    for nfr in (4, 16):
        lat, latT = _accumulate(oracle, sc, w, h, [seed(f) for f in range(1, nfr + 1)], xs=2, ys=2)
        assert (lat[..., 3][lattice(h, w, 2, 0, 0)] == nfr).all()
        for label, feat in feats.items():
            img = denoise_guided_filled(lat, feat, latT, *args)[..., :3]
            for region, where in (("metal", metal), ("glass", glass), ("all", np.ones_like(metal))):
                if where.any():
                    out[(nfr, label, region)] = _rmse(img, ref, where)
                    print(f"{name} {w}x{h} {nfr:2d} lattice frames {label:12s} {region:5s} clamped {out[(nfr, label, region)][0]:.4f} "
                          f"unclamped {out[(nfr, label, region)][1]:.4f}  ({int(where.sum())} pixels)")
    return out


def test_through_records_lift_the_filled_metal(pt, oracle):
    """C3 at 160 x 90 against a 128-frame reference, display-referred (RMSE of the clamped rgb) over the pixels whose first hit is the metal:
    lattice frames filled and filtered with the records of rule (4, 0.8, REFLECT, KEY) against the first-hit records.
    Measured with these models at 4 frames: 0.0805 against 0.1376, ratio 0.585; the bound 0.75 leaves room for small changes of the rule (the
    models are deterministic).  At 16 frames the through records give 0.0511: more frames help the filled metal now, which they did not
    (0.1376 to 0.1251 with first-hit records).  The glass figures (both lobes at 0.5) are printed, not asserted: they are mixed."""
    rules = {"reflect+key": (4, 0.8, TM.REFLECT, TM.KEY), "both 0.5": (4, 0.5, TM.REFLECT | TM.TRANSMIT, TM.KEY)}
    e = _experiment(pt, oracle, "C3", 160, 90, rules)
    r4, f4 = e[(4, "reflect+key", "metal")][0], e[(4, "first-hit", "metal")][0]
    r16 = e[(16, "reflect+key", "metal")][0]
    print(f"metal, clamped: first-hit {f4:.4f}, through {r4:.4f}, ratio {r4 / f4:.3f}; through at 16 frames {r16:.4f}")
    assert r4 / f4 < 0.75, (r4, f4)
    assert r16 < r4, (r16, r4)


def test_c6_figures_are_printed(pt, oracle):
    """C6 at 160 x 90: the reflected objects are one or two pixels wide there and the through records gain nothing (lattice metal, the materials with Pm = 1:
    0.1130 first-hit against 0.1216 at 4 frames, 0.1050 against 0.1128 at 16, with these models).  Printed, not asserted: what the rule is worth where they are wider is measured on the device."""
    e = _experiment(pt, oracle, "C6", 160, 90, {"reflect+key": (4, 0.8, TM.REFLECT, TM.KEY)})
    assert all(np.isfinite(v).all() for v in e.values())
