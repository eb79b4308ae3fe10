"""GPU: the three intersect kernels (pt_debug_intersect under extend_mode 0, 1, 2) against the float64 brute-force closest hit of
tests/_intersect_ref64.py, which reads bindings 3 and 7 and no tree — on static scenes under the layout and kernel options, after
pt_move_geometry in place, after pt_pose_geometry in place (one case per rule) and on the multi-stream slow path.

A robust ray (the margins of _intersect_ref64, all computed from the geometry) must name the reference's primitive, with t — and u, v where a
triangle wins — within BOUND_K units of tests/_intersect_cases.py (four times what tests/test_intersect_ref64.py measures for the oracle; under
the exact contract the device adds no error of its own).  A non-robust ray must equal oracle.ray_hits bit for bit: no ray goes unchecked, and
there is no cap on how many take that route.  4096 rays per set (one C2 case: 16 384, so that the persistent kernels refill); every reference is
computed once per (scene, ray set) and kept.

When a case fails the message says on how many of the offending rays the oracle agrees with the device: all of them — the tree, or the rule
that made it (builder, refit, patch), or the reference's stated rule; none — a kernel or a record."""
import numpy as np
import pytest

import _intersect_cases as IC
import _intersect_ref64 as R64
import _pose_model as PM
from test_gpu_move import context, frame
from test_gpu_parity import asm_taken

pytestmark = pytest.mark.gpu

f32 = np.float32
LAYOUTS = [dict(asm_node_layout=0), dict(asm_node_layout=1), dict(bfs_nodes=3)]
OPTIONS = [dict(asm_node_layout=0), dict(asm_node_layout=1), dict(bfs_nodes=3), dict(asm_tpb=512), dict(asm_tpb=1024), dict(stack_mode=2), dict(asm_root_cull=0),
           dict(asm_loop=0), dict(asm_loop=1)]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def tag_of(d):
    return "-".join(f"{k}{v}" for k, v in d.items()) or "default"


def sets_of(case):
    return IC.SETS + (["ellipsoids"] if int(case.buffers[7][0]) else [])


def equals_oracle(otuv, oprim, tuv, prim):
    """bool per ray: the device's hit record is the oracle's, bit for bit (u and v where a triangle wins: an ellipsoid's record keeps other words there)"""
    none = IC.missed(tuv, prim)
    tri = (oprim >= 0) & ((oprim & R64.PRIM_ELLIPSOID) == 0)
    hit = ~none & (prim == oprim) & (_bits(tuv[:, 0]) == _bits(otuv[:, 0])) & (~tri | ((_bits(tuv[:, 1]) == _bits(otuv[:, 1])) & (_bits(tuv[:, 2]) == _bits(otuv[:, 2]))))
    return np.where(oprim == -1, none, hit)


def judge(oracle, case, kind, tuv, prim, tag, n=IC.N_RAYS):
    """one hit-record array of the rays (case, kind) against the reference and, off the robust rays, against the oracle"""
    o, d, ref = IC.reference(case, kind, n)
    otuv, oprim = IC.oracle_hits(oracle, case, o, d)
    assert ref.slivers == 0, tag
    robust = ref.robust()
    as_oracle = equals_oracle(otuv, oprim, tuv, prim)
    bad = np.nonzero(robust & ~IC.same_prim(ref, tuv, prim))[0]
    assert bad.size == 0, (tag, kind, f"{bad.size} robust rays name another primitive than the reference; the oracle agrees with the device on {int(as_oracle[bad].sum())} of them",
                           [(int(i), int(ref.prim[i]), float(ref.t[i]), int(prim[i]), tuv[i].tolist()) for i in bad[:4]])
    m = np.where(robust, IC.multiples(ref, o, tuv, prim), 0.0)
    far = np.nonzero(m > IC.BOUND_K)[0]
    assert far.size == 0, (tag, kind, f"{far.size} robust rays beyond the bound; the oracle agrees with the device on {int(as_oracle[far].sum())} of them", float(m.max()),
                           [(int(i), float(ref.t[i]), float(ref.u[i]), float(ref.v[i]), tuv[i].tolist()) for i in far[:4]])
    off = np.nonzero(~robust & ~as_oracle)[0]
    assert off.size == 0, (tag, kind, f"{off.size} non-robust rays differ from the oracle", [(int(i), int(oprim[i]), otuv[i].tolist(), int(prim[i]), tuv[i].tolist()) for i in off[:4]])
    if kind in ("random", "interior"):
        assert robust.mean() >= 0.95, (tag, kind, float(robust.mean()))
    return int(robust.sum())


def probe(oracle, r, case, tag, kinds=None, n=IC.N_RAYS):
    """every ray set of the scene through the context's current intersect kernel"""
    for kind in kinds or sets_of(case):
        o, d = IC.rays(case, kind, n)
        tuv, prim = r.debug_intersect(o, d)
        judge(oracle, case, kind, tuv, prim, tag, n)


def handwritten(r, expected=True):
    """mode 2 is meant: the scene is one the hand-written kernel takes, and it has been launched"""
    assert asm_taken(r) == expected
    if expected:
        r.set_option("query_asm_launches_above", 0)


def loaded(renderer_mod, case, **opts):
    r = renderer_mod.Renderer(*case.size)
    for k, v in opts.items():
        r.set_option(k, v)
    for k, a in case.buffers.items():
        r.set_buffer(k, a)
    for i, t in case.tex.items():
        r.set_texture(i, t)
    return r


def all_modes(oracle, r, case, tag, asm=True):
    for mode in (0, 1, 2):
        r.set_option("extend_mode", mode)
        probe(oracle, r, case, (tag, mode))
    handwritten(r, asm)


# ------------------------------------------------------------------------------------------------ static scenes

@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", list(IC.STATIC))
def test_static_scenes_under_the_three_kernels(pt, oracle, renderer_mod, name, mode):
    case = IC.static(pt, name)
    r = loaded(renderer_mod, case)
    r.set_option("extend_mode", mode)
    probe(oracle, r, case, (name, mode))
    if mode == 2:
        handwritten(r)
    r.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_16384_rays_so_that_the_persistent_kernels_refill(pt, oracle, renderer_mod, mode):
    case = IC.static(pt, "C2")
    r = loaded(renderer_mod, case)
    r.set_option("extend_mode", mode)
    probe(oracle, r, case, ("C2 x 16384", mode), kinds=["interior"], n=16384)
    if mode == 2:
        handwritten(r)
    r.close()


@pytest.mark.parametrize("opts", OPTIONS, ids=[tag_of(o) for o in OPTIONS])
@pytest.mark.parametrize("name", ["C3", "C6"])
def test_the_handwritten_kernel_under_its_options(pt, oracle, renderer_mod, name, opts):
    case = IC.static(pt, name)
    r = loaded(renderer_mod, case, **opts)
    r.set_option("extend_mode", 2)
    probe(oracle, r, case, (name, opts))
    handwritten(r)
    r.close()


# ------------------------------------------------------------------------------------------------ after move_geometry in place

def moved_in_place(pt, renderer_mod, old, new, ellip=None, **opts):
    r = context(renderer_mod, old.buffers, old.tex, old.size, **opts)
    frame(pt, r, 1)
    plan = renderer_mod.RefitPlan(old.buffers)
    assert r.move_geometry(plan, new.buffers[3], ellip)[1] is True
    return r, plan


@pytest.mark.parametrize("opts", LAYOUTS, ids=[tag_of(o) for o in LAYOUTS])
@pytest.mark.parametrize("name", IC.MOVED)
def test_after_a_move_in_place(pt, oracle, renderer_mod, name, opts):
    """(emptyleaf: a leaf without triangles keeps a scene on the compiled persistent kernel)"""
    old, new = IC.moved(pt, name)
    r, plan = moved_in_place(pt, renderer_mod, old, new, **opts)
    r.set_option("extend_mode", 2)
    probe(oracle, r, new, (name, opts))
    handwritten(r, name != "emptyleaf")
    plan.close(); r.close()


def test_after_each_of_three_successive_moves(pt, oracle, renderer_mod):
    old = IC.moved(pt, "soup257")[0]
    r = context(renderer_mod, old.buffers, old.tex, old.size)
    frame(pt, r, 1)
    plan = renderer_mod.RefitPlan(old.buffers)
    r.set_option("extend_mode", 2)
    for seed in (7, 8, 9):
        new = IC.moved(pt, "soup257", seed)[1]
        assert r.move_geometry(plan, new.buffers[3])[1] is True
        probe(oracle, r, new, ("soup257", seed))
    handwritten(r)
    plan.close(); r.close()


def test_after_a_move_of_m1_with_its_ellipsoid(pt, oracle, renderer_mod):
    old, new = IC.m1(pt, 4)
    assert not np.array_equal(old.buffers[7], new.buffers[7])
    r, plan = moved_in_place(pt, renderer_mod, old, new, ellip=new.buffers[7])
    r.set_option("extend_mode", 2)
    probe(oracle, r, new, "M1@4")
    handwritten(r)
    plan.close(); r.close()


# ------------------------------------------------------------------------------------------------ after pose_geometry in place, one case per rule

def posed_case(old, pose, X, name):
    """the scene the reference judges: the pose's own triangles as downloaded (the tests of the rules hold them to the models), under the binding 10
    the refit model gives them (for the oracle's part: the tests of include/pt_move.h hold the device's refit to that model byte for byte)"""
    tris = pose.triangles(X)
    assert not np.isnan(tris).any()
    return IC.Case(name, IC.refit_onto(old.buffers, tris), old.tex, old.size)


def pose_steps(pt, oracle, renderer_mod, old, create, steps, name):
    """steps: [(X, prepare(pose) or None)].  After every step the hand-written kernel; after the last all three kernels, and once more after
    asm_node_layout = 1 rebuilt the scene from the settled copies (these trees get the 80-byte records by default)"""
    r = context(renderer_mod, old.buffers, old.tex, old.size)
    frame(pt, r, 1)
    pose = create(r)
    r.set_option("extend_mode", 2)
    for k, (X, prepare) in enumerate(steps):
        if prepare:
            prepare(pose)
        assert r.pose_geometry(pose, X)[1] is True
        case = posed_case(old, pose, X, f"{name} step {k}")
        assert not np.array_equal(case.buffers[3], old.buffers[3])
        probe(oracle, r, case, (name, k))
    handwritten(r)
    all_modes(oracle, r, case, (name, "last step"))
    r.set_option("asm_node_layout", 1)
    all_modes(oracle, r, case, (name, "rebuilt from the settled copies"))
    pose.close(); r.close()


def test_after_a_pose_by_parts(pt, oracle, renderer_mod):
    old = IC.moved(pt, "soup129")[0]
    n = old.buffers[3].size // 40
    pose_steps(pt, oracle, renderer_mod, old, lambda r: r.pose_create(PM.parts_mod4(n), 3), [(PM.matrices(3), None)], "soup129 parts")


def test_after_a_linear_skin(pt, oracle, renderer_mod):
    rest, bone, weight, X2 = pt.scenes.m3_bending(2)
    old = IC.Case("M3", *IC.MC.workload_inputs(rest), (rest.W, rest.H))
    pose_steps(pt, oracle, renderer_mod, old, lambda r: r.skin_create(bone, weight, 5), [(X2, None), (pt.scenes.m3_bending(6)[3], None)], "M3")


def test_after_morph_skin_and_normals(pt, oracle, renderer_mod):
    rest, bone, weight, targets, X3, w3, ids, nv = pt.scenes.m5_rippling(3)
    X7, w7 = pt.scenes.m5_rippling(7)[4:6]
    old = IC.Case("M5", *IC.MC.workload_inputs(rest), (rest.W, rest.H))

    def create(r):
        pose = r.skin_create(bone, weight, 5)
        pose.morph_attach(targets)
        pose.normals_attach(ids, nv)
        return pose
    pose_steps(pt, oracle, renderer_mod, old, create, [(X3, lambda p: p.morph_weights(w3)), (X7, lambda p: p.morph_weights(w7))], "M5")


def test_after_a_dual_quaternion_skin(pt, oracle, renderer_mod):
    rest, bone, weight, X2 = pt.scenes.m6_twisting(2)
    old = IC.Case("M6", *IC.MC.workload_inputs(rest), (rest.W, rest.H))
    pose_steps(pt, oracle, renderer_mod, old, lambda r: r.skin_create(bone, weight, 5, blend="dq"), [(X2, None), (pt.scenes.m6_twisting(5)[3], None)], "M6")


# ------------------------------------------------------------------------------------------------ the multi-stream slow path

def test_the_multi_stream_slow_path(pt, oracle, renderer_mod):
    """devices = [0, 0], M5 at step 7: the pose goes through the host (in_place is False); the probe runs on the first stream"""
    rest, bone, weight, targets, X, w, ids, nv = pt.scenes.m5_rippling(7)
    old = IC.Case("M5", *IC.MC.workload_inputs(rest), (rest.W, rest.H))
    r = renderer_mod.Renderer(rest.W, rest.H, devices=[0, 0])
    r.load_workload(rest)
    frame(pt, r, 1)
    pose = r.skin_create(bone, weight, 5)
    pose.morph_attach(targets)
    pose.normals_attach(ids, nv)
    pose.morph_weights(w)
    assert r.pose_geometry(pose, X)[1] is False
    case = posed_case(old, pose, X, "M5 step 7, two streams")
    r.set_option("extend_mode", 2)
    probe(oracle, r, case, "two streams")
    assert asm_taken(r)
    pose.close(); r.close()
