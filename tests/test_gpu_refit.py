"""GPU: the BVH refit (pt_refit_create, pt_refit_run, pt_refit_destroy; include/pt_refit.h) against the numpy model of tests/_refit_model.py, bit for
bit in the boxes and in root_cost; a rendered parity check on a refit tree; one plan over several poses; the refusals; the moving-geometry workflow
of include/pt_motion.h with the refit in place of the rebuild."""
import ctypes as C

import numpy as np
import pytest

import _refit_cases as RC
import _refit_model as RM
from test_gpu_parity import assert_same, render_both

pytestmark = pytest.mark.gpu

f32 = np.float32
EXTRA = [f"soup{n}" for n, _, _ in RC.SOUPS] + ["ladder", "chain256", "loose"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _same(got, want, tag):
    data, cost = got
    assert np.array_equal(_bits(data), _bits(want[0])), (tag, int((_bits(data) != _bits(want[0])).sum()))
    assert np.array_equal(cost.view(np.uint64), want[1].view(np.uint64)), (tag, cost, want[1])


def _device(renderer_mod, b, tris):
    plan = renderer_mod.RefitPlan(b)
    try:
        return plan.run(tris)
    finally:
        plan.close()


@pytest.mark.parametrize("name", EXTRA)
def test_device_equals_the_model_on_soups_ladders_and_two_objects(pt, renderer_mod, name):
    """the scene's own triangles (the identity of tests/test_refit_model.py, the chain's stale boxes apart) and a deformed copy of them.  The soups
    are two objects with continued ids; soup128, soup129 and soup257 have 256 / 258 / 514 leaves and 254 / 256 / 512 inner nodes, on both sides
    of a 256-lane block and of the one-block tail; soup1000 has launches of their own below the tail; the builder's ladder has 180 heights and
    the hand-made chain 256, each all in the tail's one launch."""
    b = RC.extra(pt)[name]
    counts = {"soup128": (256, 254), "soup129": (258, 256), "soup257": (514, 512), "ladder": (181, 180), "chain256": (257, 256)}
    if name in counts:
        height = RM.structure(b[10], b[11], b[13])[1]
        assert (int((height == 0).sum()), int((height > 0).sum())) == counts[name]
    for tris in (b[3], RC.perturbed(b[3], 7)):
        _same(_device(renderer_mod, b, tris), RM.refit_buffers(b, tris), name)
    if name != "chain256":
        assert np.array_equal(_bits(_device(renderer_mod, b, b[3])[0]), _bits(b[10]))
    if name == "soup2":
        assert int(b[13][0]) == 2 and b[13][2] > b[13][1] > -1 and b[12].max() == len(b[3]) // 40 - 1      # the second object's ids and leaf offsets continue


def test_device_equals_the_model_on_c6_with_64_roots(pt, renderer_mod):
    b = RC.workloads(pt)["C6"]
    assert int(b[13][0]) == 64
    tris = RC.perturbed(b[3], 11, 0.01)
    want = RM.refit_buffers(b, tris)
    got = _device(renderer_mod, b, tris)
    _same(got, want, "C6")
    assert len(got[1]) == 64 and (got[1] > 0).all()


@pytest.fixture(scope="module")
def m1_rest(pt):
    return pt.scenes.m1_refit(0)


@pytest.mark.parametrize("step", [1, 4, 8])
def test_m1_refit_from_the_rest_pose_topology(pt, renderer_mod, m1_rest, step):
    wl = pt.scenes.m1_refit(step)
    assert all(np.array_equal(wl.buffers[k], m1_rest.buffers[k]) for k in (10, 11, 12, 13)) and not np.array_equal(wl.buffers[3], m1_rest.buffers[3])
    want = RM.refit_buffers(wl.buffers)
    got = _device(renderer_mod, wl.buffers, wl.buffers[3])
    _same(got, want, step)
    assert not np.array_equal(_bits(got[0]), _bits(m1_rest.buffers[10]))
    # every referenced triangle lies inside the union of the refit root boxes
    v = RM.vertices(wl.buffers[3])
    roots = got[0].reshape(-1, 8)[wl.buffers[13][1:1 + int(wl.buffers[13][0])]]
    used = np.unique(wl.buffers[12])
    assert (v[used] >= roots[:, 0:3].min(axis=0)).all() and (v[used] <= roots[:, 3:6].max(axis=0)).all()


def test_render_on_the_refit_tree_is_bit_identical_to_the_oracle(pt, oracle, renderer_mod):
    """2 frames at 96 x 54 on M1 at step 4 over the rest pose's topology with refit boxes: the counting kernels and the shipped kernels (render_both
    renders with both and compares them) against the oracle on the same buffers"""
    wl = pt.scenes.m1_refit(4)
    plan = renderer_mod.RefitPlan(wl.buffers)
    wl.buffers[10], _ = plan.run(wl.buffers[3])
    plan.close()
    assert not np.array_equal(_bits(wl.buffers[10]), _bits(pt.scenes.m1_moving(0).buffers[10]))
    got, ref, cnt, ocnt = render_both(pt, oracle, renderer_mod, wl, 2)
    assert_same(got, ref, cnt, ocnt)
    assert got[..., :3].max() > 0


def test_one_plan_run_three_times_gives_what_three_fresh_plans_give(pt, renderer_mod):
    b = RC.extra(pt)["soup1000"]
    poses = [RC.perturbed(b[3], s, 0.1) for s in (1, 2)] + [b[3]]
    plan = renderer_mod.RefitPlan(b)
    kept = [tuple(a.copy() for a in plan.run(t)) for t in poses]
    plan.close()
    for t, got in zip(poses, kept):
        _same(got, _device(renderer_mod, b, t), "fresh plan")
    assert not np.array_equal(_bits(kept[0][0]), _bits(kept[1][0])) and np.array_equal(_bits(kept[2][0]), _bits(b[10]))


def test_nan_refusal_leaves_the_output_untouched_and_the_plan_usable(pt, renderer_mod):
    b = RC.extra(pt)["loose"]
    plan = renderer_mod.RefitPlan(b)
    out = np.full(b[10].size, 123.25, f32)
    cost = np.full(2, -7.0, np.float64)
    bad = b[3].copy()
    bad[40 * int(b[12][5]) + 9] = np.nan                           # a referenced triangle's third vertex
    L = renderer_mod.lib()
    assert L.pt_refit_run(plan._h, bad.ctypes.data, bad.nbytes, out.ctypes.data, cost.ctypes.data) == -4
    assert b"NaN" in L.pt_last_error()
    assert (out == f32(123.25)).all() and (cost == -7.0).all()
    with pytest.raises(renderer_mod.PtError) as e:
        plan.run(bad, out=out)
    assert e.value.code == -4 and (out == f32(123.25)).all()
    ok = b[3].copy()
    ok[0:3] = np.nan                                               # triangle 0 is loose: no leaf references it
    ok[40 * int(b[12][5]) + 3] = np.nan                            # float 3 of a referenced record is no vertex
    ok[40 * int(b[12][5]) + 4] = np.inf                            # an infinity is allowed
    got = plan.run(ok)
    want = RM.refit_buffers(b, ok)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.isinf(got[0]).any()
    _same(plan.run(b[3]), RM.refit_buffers(b), "after the refusal")
    plan.close()


def _create(L, data, tree, leaf, roots, n_tris, sizes=None, nulls=()):
    arrs = [np.ascontiguousarray(data, f32), np.ascontiguousarray(tree, np.int32), np.ascontiguousarray(leaf, np.int32), np.ascontiguousarray(roots, np.int32)]
    sizes = sizes or [a.nbytes for a in arrs]
    h = C.c_void_p()
    args = []
    for k, a in enumerate(arrs):
        args += [None if k in nulls else a.ctypes.data, sizes[k]]
    rc = L.pt_refit_create(0, *args, n_tris, C.byref(h))
    return rc, h, L.pt_last_error().decode()


def test_every_create_time_refusal_once_through_ctypes(pt, renderer_mod):
    from test_refit_model import _hand_tree
    L = renderer_mod.lib()
    data, tree, leaf, roots = _hand_tree()

    def edited(which, index, value):
        a = [data.copy(), tree.copy(), leaf.copy(), roots.copy()]
        a[which][index] = value
        return a

    cases = [
        (-1, "null buffer", dict(nulls=(2,))),
        (-1, "data_bytes is not a multiple of 32", dict(sizes=[data.nbytes - 4, tree.nbytes, leaf.nbytes, roots.nbytes])),
        (-1, "tree_bytes is not a multiple of 12", dict(sizes=[data.nbytes, tree.nbytes - 4, leaf.nbytes, roots.nbytes])),
        (-1, "leaf_bytes is not a multiple of 4", dict(sizes=[data.nbytes, tree.nbytes, leaf.nbytes - 2, roots.nbytes])),
        (-1, "roots_bytes must be a multiple of 4", dict(sizes=[data.nbytes, tree.nbytes, leaf.nbytes, 0])),
        (-1, "n_tris is negative", dict(n_tris=-1)),
        (-1, "more than 2^27 nodes", dict(n_tris=(1 << 30) + 1)),
        (-4, "shorter than 8 floats per BVHtree node", dict(sizes=[data.nbytes - 32, tree.nbytes, leaf.nbytes, roots.nbytes])),
        (-4, "row whose id is not its index", dict(arrs=edited(1, 3 * 4, 3))),
        (-4, "one child without the other", dict(arrs=edited(1, 3 * 1 + 2, -1))),
        (-4, "child outside (id, n_nodes)", dict(arrs=edited(1, 3 * 1 + 1, 0))),
        (-4, "objIndices[0] exceeds the buffer", dict(arrs=edited(3, 0, 2))),
        (-4, "root out of range", dict(arrs=edited(3, 1, 6))),
        (-4, "two parents or reached from two roots", dict(arrs=edited(1, 3 * 1 + 2, 4))),
        (-4, "is not integral", dict(arrs=edited(0, 8 * 4 + 7, 2.5))),
        (-4, "outside 0 <= start <= end <= leaf count", dict(arrs=edited(0, 8 * 4 + 7, 4.0))),
        (-4, "entry outside [0, n_tris)", dict(arrs=edited(2, 1, 3))),
    ]
    for rc_want, text, kw in cases:
        arrs = kw.pop("arrs", [data, tree, leaf, roots])
        rc, h, msg = _create(L, *arrs, kw.pop("n_tris", 3), **kw)
        assert rc == rc_want and text in msg and msg.startswith("pt_refit_create: ") and not h.value, (text, rc, msg)
    # two roots over one node: the same text from the roots' side
    rc, h, msg = _create(L, data, tree, leaf, np.array([2, 0, 0], np.int32), 3)
    assert rc == -4 and "two parents or reached from two roots" in msg
    assert L.pt_refit_create(0, data.ctypes.data, data.nbytes, tree.ctypes.data, tree.nbytes, leaf.ctypes.data, leaf.nbytes, roots.ctypes.data, roots.nbytes, 3, None) == -1
    rc, h, msg = _create(L, data, tree, leaf, roots, 3)
    assert rc == 0 and h.value
    # the run-time refusals, and a plan that is gone
    tris = np.zeros(3 * 40, f32)
    out = np.zeros(data.size, f32)
    assert L.pt_refit_run(h, tris.ctypes.data, tris.nbytes - 160, out.ctypes.data, None) == -1 and b"tri_bytes" in L.pt_last_error()
    assert L.pt_refit_run(h, None, tris.nbytes, out.ctypes.data, None) == -1
    assert L.pt_refit_run(h, tris.ctypes.data, tris.nbytes, None, None) == -1
    assert L.pt_refit_run(None, tris.ctypes.data, tris.nbytes, out.ctypes.data, None) == -1
    assert not out.any()
    assert L.pt_refit_run(h, tris.ctypes.data, tris.nbytes, out.ctypes.data, None) == 0                # root_cost may be NULL
    assert np.array_equal(_bits(out), _bits(RM.refit(data, tree, leaf, roots, tris)[0]))
    L.pt_refit_destroy(h)
    assert L.pt_refit_run(h, tris.ctypes.data, tris.nbytes, out.ctypes.data, None) == -1 and b"destroyed" in L.pt_last_error()
    L.pt_refit_destroy(h)                                          # a second destroy and a null one are ignored
    L.pt_refit_destroy(None)
    rc, h2, msg = _create(L, data, tree, leaf, roots, 3)
    assert rc == 0
    assert L.pt_refit_create(99, data.ctypes.data, data.nbytes, tree.ctypes.data, tree.nbytes, leaf.ctypes.data, leaf.nbytes, roots.ctypes.data, roots.nbytes, 3,
                             C.byref(C.c_void_p())) == -2
    L.pt_refit_destroy(h2)


def test_moving_geometry_workflow_end_to_end_on_m1(pt, renderer_mod):
    """render 4 frames, mark, move_triangles plus binding 7, reproject: plumbing only.  Equality with a rebuilt-tree twin is not asserted, because
    coplanar ties may resolve differently in another tree."""
    W, H = 96, 54
    rest, moved = pt.scenes.m1_moving(0, W, H), pt.scenes.m1_moving(2, W, H)
    r = renderer_mod.Renderer(W, H)
    r.load_workload(rest)
    r.reset_frame()
    r.render_batch(1, [pt.scenes.frame_seed(f) for f in range(1, 5)])
    plan = renderer_mod.RefitPlan(rest.buffers)
    _, rest_cost = plan.run(rest.buffers[3])
    r.motion_mark()
    data, cost = r.move_triangles(plan, moved.buffers[3])
    r.set_buffer(7, moved.buffers[7])
    kept = r.reproject_frame_moved()
    assert 0 < kept <= W * H
    assert np.array_equal(_bits(data), _bits(RM.refit(rest.buffers[10], rest.buffers[11], rest.buffers[12], rest.buffers[13], moved.buffers[3])[0]))
    assert cost.shape == rest_cost.shape and (cost > 0).all()
    r.render_batch(5, [pt.scenes.frame_seed(5)])                    # the next render takes the refit buffers like any upload
    fr = r.read_frame()
    assert np.isfinite(fr[..., 3]).all() and fr[..., 3].max() > 4
    plan.close()
    r.close()
