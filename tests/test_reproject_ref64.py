"""CPU: the four float32 reprojection twins (tests/_reproject_model.py, _reproject_bilinear_model.py, _motion_model.py, _motion_bilinear_model.py)
against the float64 scene-space reference of tests/_reproject_ref64.py, on the records _cpu_features makes from the oracle's rayScene, for the
cases of tests/_reproject_cases.py; tests/test_gpu_reproject_ref64.py holds k_reproject to the same reference on the device's own records.

The twins restate include/pt_reproject.h line by line and the kernel is held to them bit for bit, so a mistake the header, a twin and the kernel
share passes every other test.  The reference reads the scene and the two cameras only.  Every case runs the nearest rule and the bilinear rule
at snap 1/64 and 0, each at max_history 64 and 4 (the cap), with normal_tol = -1 and depth_tol 0.02.

Measured (this module prints every figure):
  disagreements on decided pixels, in the decision or in the source, over the 13 cases x 3 rules x 2 caps          0
  K, the largest of |mean - ref| / unit and |a - ref| / (7 unit) over the decided kept pixels, unit = (unit_x + unit_y) / Ws of
  tests/_reproject_ref64.compare                                   47.56 (pixel (96, 1) of C2dolly, 100 x 7, snap 1/64, max_history 64)
  the bound                                                        BOUND_K = 4 K = 190.2 units
  decided share of the nearest rule, from the reference alone      SHARES below: 96.2 % on C2 and 93.9 % on C3 (90 % required)
K is nearly all one term: the records' t is counted from o + 1e-4 d and step 2 of the header adds it to o, so the twins' P lies 1e-4 short of
the surface along the new ray; with the reference's points moved back by as much the largest multiple over C2, C6 and C2dolly is 0.56.  That is
2.1e-4 px under the small move at 96 across (the 2.2e-4 px a prototype of this reference reported as its raw maximum) and 1.0e-3 px under the
dolly.  The nearest rule below the cap copies (K = 0 exactly); at the cap the rescaling's rounding gives 0.28.
Against the prototype: materials come from bindings 3 and 7, never from a record (its four apparent wrong keeps on C2 do not occur); C6 runs at
65 x 17, since its 8192 triangles took the brute force 30 s at 96 x 54.
Mutations of a copy of a twin (never of product code), each noticed as disagreements on decided pixels: MUTATIONS below."""
import inspect
import types

import numpy as np
import pytest

import _motion_bilinear_model as MBM
import _motion_model as MM
import _reproject_bilinear_model as RBM
import _reproject_cases as RC
import _reproject_model as RM
import _reproject_ref64 as RR
from _intersect_cases import _once
from test_fill_abi import _cpu_features

f32 = np.float32
CAPS = (64.0, 4.0)
RULES = ("nearest",) + RC.SNAPS
FEATURES_OF = {"C3all": "C3"}


def test_projection_inverts_the_camera_under_a_full_rotation():
    """every pixel centre of a camera with all three angles non-zero, pushed along its ray to a point and taken as a direction, comes back to
    (x + 0.5, y + 0.5) within 1e-9 px, with q2 > 0; the opposite direction lies behind"""
    W, H = 96, 54
    cam = RR.Camera((0.3, 1.0, -1.6), (0.15, -0.4, 0.3), [1.5, 1.0, W, H / W])
    d = cam.dirs(W, H)
    y, x = np.mgrid[0:H, 0:W]
    for X in (d, 2.75 * d):
        sx, sy, q2 = RR.project(X, cam, W, H)
        assert np.abs(sx - (x + 0.5)).max() < 1e-9 and np.abs(sy - (y + 0.5)).max() < 1e-9 and (q2 > 0).all()
    assert (RR.project(-d, cam, W, H)[2] < 0).all()
    assert not np.allclose(cam.M, cam.M.T)                          # a camera whose matrix and its transpose differ


def test_probe_images_are_exact_and_name_their_taps():
    fr, T = RR.probe_images(100, 7)
    y, x = np.mgrid[0:7, 0:100]
    assert np.array_equal(fr[..., 0] / fr[..., 3], (x + 0.5).astype(f32)) and np.array_equal(fr[..., 1] / fr[..., 3], (y + 0.5).astype(f32))
    assert np.array_equal(T[..., :3], fr[..., [0, 1, 3]]) and fr[..., 3].min() == 1 and fr[..., 3].max() == RR.A_MAX
    a = fr[..., 3]
    quad = np.stack([a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:]], -1)
    assert all(len(set(q)) == 4 for q in quad.reshape(-1, 4))       # the four neighbours of any point differ in their counts


# ---------------------------------------------------------------------------------------------------------------- the twins on a case

class Twins:
    """the modules a run goes through; a mutation replaces one by a changed copy"""
    nearest, bilinear, motion = RM, RBM, MM


def _features(pt, oracle, name):
    name = FEATURES_OF.get(name, name)
    c = RC.case(pt, name)
    return _once(("reproject features", name), lambda: (_cpu_features(oracle, c.then), _cpu_features(oracle, c.now)))


def run_twin(pt, oracle, name, rule, cap, twins=Twins):
    """(FRAME, T, kept, blended) of one call's twin on the probe images"""
    c = RC.case(pt, name)
    rh, rn = _features(pt, oracle, name)
    fr, T = RR.probe_images(c.W, c.H)
    fin_a = RM.frame_in(c.then.buffers[4], *c.A, RC.NO_MOUSE)
    fin_b = RM.frame_in(c.now.buffers[4], *c.B, RC.NO_MOUSE)
    vd, M = RM.material_flags(c.now.buffers[14]), RM.cam_rot(c.A[1])
    geo = ()
    if c.moved:
        geo = (MM.tri_vertices(c.now.buffers[3]), MM.tri_vertices(c.then.buffers[3]), MM.ellipsoids(c.now.buffers[7]), MM.ellipsoids(c.then.buffers[7]))
    if twins is Twins:                                              # the twins' own entry points
        if rule == "nearest":
            out = (MM.reproject_moved(rn, rh, fr, T, fin_a, fin_b, vd, M, *geo, cap, RC.DEPTH_TOL, -1.0, c.allm) if c.moved else
                   RM.reproject(rn, rh, fr, T, fin_a, fin_b, vd, M, cap, RC.DEPTH_TOL, -1.0, c.allm))
            return out + (0,)
        if c.moved:
            return MBM.reproject_moved_bilinear(rn, rh, fr, T, fin_a, fin_b, vd, M, *geo, cap, RC.DEPTH_TOL, -1.0, rule, c.allm)
        return RBM.reproject_bilinear(rn, rh, fr, T, fin_a, fin_b, vd, M, cap, RC.DEPTH_TOL, -1.0, rule, c.allm)
    r, fin = twins.motion.mapped_records(rn, fin_b, *geo) if c.moved else (rn, fin_b)      # the same composition over the copies
    if rule == "nearest":
        return twins.nearest.reproject(r, rh, fr, T, fin_a, fin, vd, M, cap, RC.DEPTH_TOL, -1.0, c.allm) + (0,)
    return twins.bilinear.reproject_bilinear(r, rh, fr, T, fin_a, fin, vd, M, cap, RC.DEPTH_TOL, -1.0, rule, c.allm)


def found(pt, oracle, name, rule, cap, twins=Twins):
    out, tout, kept, blended = run_twin(pt, oracle, name, rule, cap, twins)
    f = RR.compare(RC.expect(pt, name, rule), out, tout, cap)
    f.kept, f.blended, f.out = kept, blended, out
    return f


# ---------------------------------------------------------------------------------------------------------------- shares, agreement, K

# name: (decided share of the nearest rule, kept share of the decided pixels), measured from the reference alone.  Asserted: C2 and C3 at least
# 0.90 decided; every case at least its recorded share less 0.05.  C2yaw2, C2dolly, M1ellrot and C1 are the cases with a built-in share of
# rejections or of sky: their floors are their own recorded figures by the same rule.
SHARES = {
    "C2": (0.9620, 0.9633, 0.8158, 0.8424), "C3": (0.9387, 0.8376, 0.7784, 0.8005), "C3all": (0.9321, 0.9729, 0.7407, 0.7664),
    "C1": (0.9749, 0.9001, 0.8019, 0.8495), "C6": (0.8860, 0.5720, 0.6769, 0.7005), "C2roll": (0.9710, 0.8239, 0.8778, 0.8986),
    "C2dolly": (0.9371, 0.9787, 0.7314, 0.7714), "C2yaw2": (0.9982, 0.0045, 0.9982, 0.9991), "M1": (0.9784, 0.9923, 0.0666, 0.0677),
    "M1cam": (0.9587, 0.9686, 0.8059, 0.8341), "M5": (0.9620, 0.9711, 0.8021, 0.8329), "M1ell": (0.9819, 0.9978, 0.0226, 0.0245),
    "M1ellrot": (0.9819, 0.9619, 0.0276, 0.0276),
}
SKY = {"C1": 0.9628, "C2roll": 0.8185}         # the share of the sky pixels that are decided and kept: a miss onto a miss
FLOOR = {"C2": 0.90, "C3": 0.90}


@pytest.mark.parametrize("name", RC.NAMES)
def test_decided_share(pt, name):
    """from the reference alone, before any model or kernel runs"""
    ref = RC.reference(pt, name)
    e = RC.expect(pt, name, "nearest")
    share, kept = float(e.decided.mean()), float((e.decided & e.kept).sum() / max(1, e.decided.sum()))
    b = [RC.expect(pt, name, s) for s in RC.SNAPS]
    print(f"{name} {ref.W}x{ref.H}: hits {ref.new.is_hit.mean():.3f}, robust new {ref.new.robust.mean():.3f} old {ref.old.robust.mean():.3f}; nearest decided "
          f"{share:.4f}, kept {kept:.4f} of them; bilinear decided " + ", ".join(f"{x.decided.mean():.4f} (four taps {((x.taps == 4) & x.decided).mean():.3f})" for x in b))
    assert share >= FLOOR.get(name, 0.0)
    miss = ~ref.new.is_hit.reshape(ref.H, ref.W)
    if miss.any():
        sky = float((miss & e.decided & e.kept).sum() / miss.sum())
        print(f"{name}: {int(miss.sum())} pixels of sky, decided and kept (a miss onto a miss) {sky:.4f}")
        assert sky >= SKY.get(name, 0.0) - 0.05, (name, sky)
    if name in SHARES:
        want_share, want_kept = SHARES[name][:2]
        assert share >= want_share - 0.05 and abs(kept - want_kept) <= 0.05, (name, share, kept)
        for x, want in zip(b, SHARES[name][2:]):
            assert x.decided.mean() >= want - 0.05, (name, float(x.decided.mean()), want)


@pytest.mark.parametrize("name", RC.NAMES)
def test_the_twins_agree_with_the_reference(pt, oracle, name):
    """0 disagreements on decided pixels, in the decision and in the source, under every rule and cap; every multiple within the bound"""
    for rule in RULES:
        for cap in CAPS:
            f = found(pt, oracle, name, rule, cap)
            print(f"{name} {rule} cap {cap:g}: decided {f.n_decided}, kept {f.n_kept} (twin kept {f.kept}, blended {f.blended}), wrong decision {f.wrong_decision}, "
                  f"wrong source {f.wrong_source}, K {f.k:.2f} at {f.where}")
            assert f.disagreements() == 0, (name, rule, cap, f.wrong_decision, f.wrong_source)
            assert f.k <= RC.BOUND_K, (name, rule, cap, f.k, f.where)
            assert f.kept == int((f.out[..., 3] > 0).sum())


def test_the_recorded_k_is_the_measured_one(pt, oracle):
    ks = {(n, r, c): found(pt, oracle, n, r, c) for n in RC.NAMES for r in RULES for c in CAPS}
    key = max(ks, key=lambda k: ks[k].k)
    print(f"K {ks[key].k:.3f}: {key} at pixel {ks[key].where}")
    assert 0.99 * RC.MEASURED_K <= ks[key].k <= RC.MEASURED_K and RC.BOUND_K == 4.0 * RC.MEASURED_K, (key, ks[key].k)


# ---------------------------------------------------------------------------------------------------------------- mutations

Q_ROW = "q = [(v0 * M[3 * i] + v1 * M[3 * i + 1]) + v2 * M[3 * i + 2] for i in range(3)]"
Q_COL = "q = [(v0 * M[i] + v1 * M[3 + i]) + v2 * M[6 + i] for i in range(3)]"
# name: [(twin, the text, its replacement)]
MUTATIONS = {
    "M' transposed": [("nearest", Q_ROW, Q_COL), ("bilinear", Q_ROW, Q_COL)],
    "hr' dropped": [("nearest", "b / (hr * ss)", "b / ss"), ("bilinear", "b / (hr * ss)", "b / ss")],
    "x mirror dropped": [("nearest", "(f32(1) - a / ss)", "(f32(1) + a / ss)"), ("bilinear", "(f32(1) - a / ss)", "(f32(1) + a / ss)")],
    "- 0.5 dropped from the tap rule": [("bilinear", "f = (s - f32(0.5)).astype(f32)", "f = s.astype(f32)")],
    "tap weights of x and y exchanged": [("bilinear", "w = (ax[i] * ay[j]).astype(f32)", "w = (ax[j] * ay[i]).astype(f32)")],
    "beta and gamma exchanged": [("motion", "pp = (Ah + beta[:, None] * h1) + gamma[:, None] * h2", "pp = (Ah + gamma[:, None] * h1) + beta[:, None] * h2")],
    "ellipsoid k inverted": [("motion", "kk = np.sqrt(now[:, 3:6] / then[:, 3:6]) * (then[:, 9] / now[:, 9])[:, None]",
                              "kk = np.sqrt(then[:, 3:6] / now[:, 3:6]) * (now[:, 9] / then[:, 9])[:, None]")],
    "depth against the new t": [("nearest", "ln = np.sqrt((v0 * v0 + v1 * v1) + v2 * v2)", "ln = t"),
                                ("bilinear", "ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])", "ln = rn[:, 0]")],
}


def _copy(module, edits):
    src = inspect.getsource(module)
    for old, new in edits:
        assert src.count(old) == 1, (module.__name__, old)
        src = src.replace(old, new)
    out = types.ModuleType(module.__name__ + "_copy")
    exec(compile(src, module.__file__, "exec"), out.__dict__)
    return out


def mutant(name):
    t = types.SimpleNamespace(nearest=RM, bilinear=RBM, motion=MM)
    for which in {w for w, _, _ in MUTATIONS[name]}:
        setattr(t, which, _copy(getattr(Twins, which), [(o, n) for w, o, n in MUTATIONS[name] if w == which]))
    return t


def test_an_unchanged_copy_is_the_twin(pt, oracle):
    """the composition the mutants run through, over unchanged copies, gives the twins' own results bit for bit"""
    t = types.SimpleNamespace(nearest=_copy(RM, []), bilinear=_copy(RBM, []), motion=_copy(MM, []))
    for name in ("C2roll", "M1cam"):
        for rule in RULES:
            a, b = run_twin(pt, oracle, name, rule, 64.0), run_twin(pt, oracle, name, rule, 64.0, t)
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[2:] == b[2:]


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_a_mutation_is_noticed(pt, oracle, name):
    t = mutant(name)
    twins = {w for w, _, _ in MUTATIONS[name]}
    rules = list(RC.SNAPS) if twins == {"bilinear"} else list(RULES)
    seen = {}
    for case in RC.NAMES:
        if twins == {"motion"} and not RC.case(pt, case).moved:
            continue
        for rule in rules:
            n = found(pt, oracle, case, rule, 64.0, t).disagreements()
            if n:
                seen[(case, rule)] = n
    print(f"{name}: disagreements on decided pixels {seen}")
    assert seen, name
