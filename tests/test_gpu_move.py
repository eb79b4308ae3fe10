"""GPU: pt_move_geometry (include/pt_move.h) — after the call a context's device record arrays, read back through pt_debug_scene_records, equal byte
for byte what a fresh context builds from the new bindings; the rendered frames are the oracle's and a move_triangles twin's; the moving-geometry
workflow of include/pt_motion.h; the slow paths; the refusals, which leave records and image as they were.  48 x 27 or 96 x 54, a few frames."""
import ctypes as C

import numpy as np
import pytest

import _move_cases as MC
import _refit_cases as RC
import _refit_model as RM
from test_gpu_parity import assert_same, seeds_for

pytestmark = pytest.mark.gpu

f32 = np.float32
ARRAYS = ("nodes", "nodes80", "tris", "shade", "roots", "ellip", "triObj")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def context(renderer_mod, b, tex, size, **opts):
    r = renderer_mod.Renderer(*size)
    for k, v in opts.items():
        r.set_option(k, v)
    for k, a in b.items():
        r.set_buffer(k, a)
    for i, t in tex.items():
        r.set_texture(i, t)
    r.reset_frame()
    return r


def frame(pt, r, f=1, n=1):
    """frames f .. f+n-1 alone in the image"""
    r.reset_frame()
    r.render_batch(f, seeds_for(pt, f, n))
    return r.read_frame()


def records(r, skip=()):
    return {k: _bits(r.debug_scene_records(k)) for k in ARRAYS if k not in skip}


def same_records(a, b, tag):
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (tag, k, a[k].shape, b[k].shape, int((a[k] != b[k]).sum()) if a[k].shape == b[k].shape else -1)


def same_image(a, b, tag):
    assert ((a == b) | (np.isnan(a) & np.isnan(b))).all(), tag


_model = {}


def model(old, new):
    """the numpy model's (binding 10, root_cost) for the move, once per new binding 3"""
    key = id(new[3])
    if key not in _model:
        _model[key] = (new[3], RM.refit(old[10], old[11], old[12], old[13], new[3]))
    return _model[key][1]


def moved_equals_fresh(pt, renderer_mod, old, new, tex, size, tag, ellip=None, want_in_place=True, **opts):
    """old scene, one frame, move_geometry; every array but the ellipsoids' (whose rotation matrices the frame setup writes) is compared at once, all of
    them and the image after one more frame on both sides"""
    r = context(renderer_mod, old, tex, size, **opts)
    frame(pt, r, 1)
    plan = renderer_mod.RefitPlan(old)
    cost, in_place = r.move_geometry(plan, new[3], ellip)
    assert in_place == want_in_place, tag
    at_once = records(r, skip=("ellip",))
    img = frame(pt, r, 2)
    got = records(r)
    plan.close(); r.close()
    want_data, want_cost = model(old, new)
    assert np.array_equal(cost.view(np.uint64), want_cost.view(np.uint64)), tag
    assert np.array_equal(_bits(new[10]), _bits(want_data)), tag        # (the fresh context below uploads the model's binding 10)
    fresh = context(renderer_mod, new, tex, size, **opts)
    ref = frame(pt, fresh, 2)
    want = records(fresh)
    fresh.close()
    same_records(got, want, tag)
    same_records(at_once, {k: want[k] for k in at_once}, (tag, "before the next render"))
    same_image(img, ref, tag)
    return got


def scene_move(pt, name):
    old = MC.scenes(pt)[name]
    tris, data = MC.moved(pt, name)
    new = dict(old); new[3] = tris; new[10] = data
    return old, new


SMALL = ["soup2", "soup3", "soup64", "soup65", "soup128", "soup129", "soup257", "soup1000", "ladder60", "chain60", "loose", "objects70", "leafroot", "emptyleaf", "hand"]
VARIANTS = [dict(asm_node_layout=0), dict(asm_node_layout=1), dict(bfs_nodes=3), dict(asm_node_layout=0, bfs_nodes=5, asm_root_cull=0)]


@pytest.mark.parametrize("name", SMALL)
def test_records_equal_a_fresh_build(pt, renderer_mod, name):
    """soup128 / 129 / 257 have 254 / 256 / 512 inner records and two or three blocks of triangle records: both sides of a 256-lane block"""
    old, new = scene_move(pt, name)
    got = moved_equals_fresh(pt, renderer_mod, old, new, MC.SKY, (MC.W, MC.H), name)
    assert not np.array_equal(got["tris"], records_of_old(pt, renderer_mod, name)["tris"])


def test_a_vertex_at_infinity_gives_the_nan_edges_the_host_gives(pt, renderer_mod):
    old = MC.scenes(pt)["hand"]
    new = dict(old); new[3], new[10] = MC.move_of(old, MC.infinite_vertex(old[3]))
    got = moved_equals_fresh(pt, renderer_mod, old, new, MC.SKY, (MC.W, MC.H), "inf")
    assert np.isnan(got["tris"].view(f32)[:9]).any() or np.isnan(got["tris"].view(f32)[12:21]).any()


_old_records = {}


def records_of_old(pt, renderer_mod, name):
    if name not in _old_records:
        r = context(renderer_mod, MC.scenes(pt)[name], MC.SKY, (MC.W, MC.H))
        frame(pt, r, 1)
        _old_records[name] = records(r)
        r.close()
    return _old_records[name]


@pytest.mark.parametrize("opts", VARIANTS, ids=["layout0", "layout1", "bfs3", "layout0-bfs5-nocull"])
@pytest.mark.parametrize("name", ["soup129", "soup1000", "objects70", "leafroot"])
def test_records_equal_a_fresh_build_under_the_layout_options(pt, renderer_mod, name, opts):
    old, new = scene_move(pt, name)
    moved_equals_fresh(pt, renderer_mod, old, new, MC.SKY, (MC.W, MC.H), (name, opts), **opts)


@pytest.mark.parametrize("opts", [{}] + VARIANTS[:3], ids=["default", "layout0", "layout1", "bfs3"])
def test_records_equal_a_fresh_build_on_c6_with_64_roots(pt, renderer_mod, opts):
    wl = RC.workload(pt, "C6")
    old, tex = MC.workload_inputs(wl)
    assert int(old[13][0]) == 64
    tris = RC.perturbed(old[3], 11, 0.01)
    new = dict(old); new[3], new[10] = MC.move_of(old, tris)
    got = moved_equals_fresh(pt, renderer_mod, old, new, tex, (wl.W, wl.H), ("C6", opts), **opts)
    assert got["roots"].size == (64 + 64) * 8


@pytest.fixture(scope="module")
def m1(pt):
    """(rest pose, {step: moved workload over the rest pose's trees with the model's refit binding 10})"""
    rest = pt.scenes.m1_moving(0)
    steps = {}
    for s in (1, 2, 4, 8):
        wl = pt.scenes.m1_refit(s)
        wl.buffers[10] = RM.refit_buffers(wl.buffers)[0]
        steps[s] = wl
    return rest, steps


@pytest.mark.parametrize("step", [1, 4, 8])
def test_records_equal_a_fresh_build_on_m1_with_its_moved_ellipsoid(pt, renderer_mod, m1, step):
    rest, steps = m1
    old, tex = MC.workload_inputs(rest)
    new = dict(steps[step].buffers)
    moved_equals_fresh(pt, renderer_mod, old, new, tex, (rest.W, rest.H), ("M1", step), ellip=new[7])
    if step == 4:
        for opts in VARIANTS[:3]:
            moved_equals_fresh(pt, renderer_mod, old, new, tex, (rest.W, rest.H), ("M1", step, opts), ellip=new[7], **opts)


def test_rendered_parity_with_the_oracle_and_a_move_triangles_twin_on_m1(pt, oracle, renderer_mod, m1):
    """2 frames after move_geometry from the rest pose to step 4: the counting kernels, the shipped kernels, the oracle on the same buffers and a
    twin context that took move_triangles + set_buffer(7) all give the same bits"""
    rest, steps = m1
    wl = steps[4]
    old, tex = MC.workload_inputs(rest)
    seeds = seeds_for(pt, 1, 2)
    out = []
    for twin in (False, True):
        r = context(renderer_mod, old, tex, (rest.W, rest.H))
        frame(pt, r, 1)
        plan = renderer_mod.RefitPlan(old)
        if twin:
            r.move_triangles(plan, wl.buffers[3])
            r.set_buffer(7, wl.buffers[7])
        else:
            assert r.move_geometry(plan, wl.buffers[3], wl.buffers[7])[1] is True
        r.set_option("count_stats", 1)
        r.reset_frame(); r.reset_counters()
        r.render_batch(1, seeds)
        got, cnt = r.read_frame(), r.counters()
        r.set_option("count_stats", 0)
        r.reset_frame()
        r.render_batch(1, seeds)
        same_image(r.read_frame(), got, "shipped kernels against the counting variants")
        out.append((got, cnt))
        plan.close(); r.close()
    sc = oracle.Scene.from_workload(wl)
    ref, ocnt = oracle.render_frames(sc, rest.W, rest.H, 1, 2, seeds, nthreads=8)
    assert_same(out[0][0], ref, out[0][1], dict(zip(oracle.COUNTERS, [int(x) for x in ocnt])))
    same_image(out[0][0], out[1][0], "move_triangles twin")
    assert out[0][0][..., :3].max() > 0


def test_three_moves_on_one_context_end_in_the_rest_poses_records(pt, renderer_mod, m1):
    rest, steps = m1
    old, tex = MC.workload_inputs(rest)
    r = context(renderer_mod, old, tex, (rest.W, rest.H))
    frame(pt, r, 1)
    plan = renderer_mod.RefitPlan(old)
    seen = []
    for wl in (steps[1], steps[2], rest):
        assert r.move_geometry(plan, wl.buffers[3], wl.buffers[7])[1] is True
        frame(pt, r, 2)
        seen.append(records(r))
    img = frame(pt, r, 2)
    plan.close(); r.close()
    assert not np.array_equal(seen[0]["tris"], seen[1]["tris"]) and not np.array_equal(seen[0]["nodes"], seen[2]["nodes"])
    for k, wl in enumerate((steps[1], steps[2], rest)):
        fresh = context(renderer_mod, wl.buffers, tex, (rest.W, rest.H))
        ref = frame(pt, fresh, 2)
        same_records(seen[k], records(fresh), ("move", k))
        fresh.close()
    same_image(img, ref, "the rest pose again")
    assert np.array_equal(_bits(RM.refit_buffers(rest.buffers)[0]), _bits(rest.buffers[10]))      # the rest pose's refit is its own binding 10


def _workflow(pt, renderer_mod, rest, steps, tex, in_place, bilinear, running=False):
    W, H = rest.W, rest.H
    r = context(renderer_mod, rest.buffers, tex, (W, H))
    plan = renderer_mod.RefitPlan(rest.buffers)
    out = []
    first = 1
    for step in (2, 4):
        if running:
            r.render_batch_async(first, seeds_for(pt, first, 4))      # not read: the move finds the frame stream running
        else:
            r.render_batch(first, seeds_for(pt, first, 4))
            r.motion_mark()
        wl = steps[step]
        if in_place:
            assert r.move_geometry(plan, wl.buffers[3], wl.buffers[7])[1] is True
        else:
            r.move_triangles(plan, wl.buffers[3])
            r.set_buffer(7, wl.buffers[7])
        if running:
            out.append(r.read_frame().copy())
        else:
            kept = r.reproject_frame_moved_bilinear() if bilinear else r.reproject_frame_moved()
            out.append(kept)
            out.append(r.read_frame().copy())
        first += 4
    r.render_batch(first, seeds_for(pt, first, 1))
    out.append(r.read_frame().copy())
    plan.close(); r.close()
    return out


@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
def test_motion_workflow_equals_the_move_triangles_twin(pt, renderer_mod, m1, bilinear):
    """4 frames, mark, move, reproject, twice, one more frame: kept counts and FRAME equal the twin that uploaded bindings 3, 10 and 7 (the same
    trees and the same state, so equality is exact)"""
    rest, steps = m1
    tex = MC.workload_inputs(rest)[1]
    a = _workflow(pt, renderer_mod, rest, steps, tex, True, bilinear)
    b = _workflow(pt, renderer_mod, rest, steps, tex, False, bilinear)
    assert len(a) == len(b) == 5
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            same_image(x, y, k)
        else:
            assert x == y and np.all(np.asarray(x) > 0), (k, x, y)


def test_move_while_a_frame_stream_is_running(pt, renderer_mod, m1):
    rest, steps = m1
    tex = MC.workload_inputs(rest)[1]
    a = _workflow(pt, renderer_mod, rest, steps, tex, True, False, running=True)
    b = _workflow(pt, renderer_mod, rest, steps, tex, False, False, running=True)
    assert len(a) == len(b) == 3
    for k, (x, y) in enumerate(zip(a, b)):
        same_image(x, y, k)
    assert a[2][..., 3].max() > a[1][..., 3].max() > a[0][..., 3].max() > 0      # nothing was reset: 4, 8 and 9 frames


def test_slow_path_foreign_unordered_boxes(pt, renderer_mod):
    old, new = scene_move(pt, "unordered80")
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H), asm_node_layout=0)
    frame(pt, r, 1)
    with pytest.raises(renderer_mod.PtError):
        r.set_option("query_asm_eligible", 0)                       # the inverted box keeps the scene off the hand-written kernel
    r.close()
    moved_equals_fresh(pt, renderer_mod, old, new, MC.SKY, (MC.W, MC.H), "unordered80", want_in_place=False, asm_node_layout=0)
    moved_equals_fresh(pt, renderer_mod, old, new, MC.SKY, (MC.W, MC.H), "unordered64", want_in_place=True, asm_node_layout=1)


def test_slow_path_binding_7_with_another_material(pt, renderer_mod, m1):
    rest, steps = m1
    old, tex = MC.workload_inputs(rest)
    new = dict(steps[4].buffers)
    e = new[7].copy()
    assert e[0] == 1.0 and e[11] != 0.0
    e[11] = 0.0
    new[7] = e
    moved_equals_fresh(pt, renderer_mod, old, new, tex, (rest.W, rest.H), "M1 other material", ellip=e, want_in_place=False)


def test_slow_path_multi_stream_context(pt, renderer_mod, m1):
    rest, steps = m1
    wl = steps[4]
    W, H = rest.W, rest.H
    r = renderer_mod.Renderer(W, H, devices=[0, 0])
    r.load_workload(rest)
    frame(pt, r, 1)
    with pytest.raises(renderer_mod.PtError) as e:
        r.debug_scene_records("nodes")
    assert e.value.code == -1
    plan = renderer_mod.RefitPlan(rest.buffers)
    cost, in_place = r.move_geometry(plan, wl.buffers[3], wl.buffers[7])
    assert in_place is False and np.array_equal(cost.view(np.uint64), RM.refit_buffers(wl.buffers)[1].view(np.uint64))
    img = frame(pt, r, 2)
    plan.close(); r.close()
    fresh = renderer_mod.Renderer(W, H, devices=[0, 0])
    fresh.load_workload(wl)
    same_image(img, frame(pt, fresh, 2), "multi")
    fresh.close()


def test_refusals_leave_records_and_image_as_they_were_and_the_plan_usable(pt, renderer_mod):
    old, new = scene_move(pt, "loose")
    L = renderer_mod.lib()
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
    img = frame(pt, r, 1)
    before = records(r)
    plan = renderer_mod.RefitPlan(old)
    other = dict(old); other[12] = old[12].copy(); other[12][[0, 1]] = other[12][[1, 0]]
    assert not np.array_equal(other[12], old[12])
    foreign = renderer_mod.RefitPlan(other)
    gone = renderer_mod.RefitPlan(old)
    gone_handle = C.c_void_p(gone._h.value)
    gone.close()
    used = int(old[12][5])
    nan = new[3].copy(); nan[40 * used + 9] = np.nan
    mat = new[3].copy(); mat[40 * used + 36] = 99.0
    matnan = new[3].copy(); matnan[40 * used + 36] = np.nan
    loose_only = new[3].copy(); loose_only[0:3] = np.nan; loose_only[36] = 99.0      # triangle 0 is referenced by no leaf: allowed

    def call(plan_handle, tris, nbytes=None, ellip=None):
        flag = C.c_int(-5)
        cost = np.full(plan.n_roots, -7.0)
        rc = L.pt_move_geometry(r._h, plan_handle, tris.ctypes.data, tris.nbytes if nbytes is None else nbytes, None if ellip is None else ellip.ctypes.data,
                                0 if ellip is None else ellip.nbytes, cost.ctypes.data, C.byref(flag))
        return rc, L.pt_last_error().decode(), flag.value, cost

    short_ellip = np.array([1.0, 0, 0, 0], f32)
    cases = [(plan._h, nan, None, None, -4, "NaN coordinate in a referenced triangle"),
             (plan._h, mat, None, None, -4, "triangle material index out of range"),
             (plan._h, matnan, None, None, -4, "triangle material index out of range"),
             (foreign._h, new[3], None, None, -4, "not made from this context's scene"),
             (plan._h, new[3], new[3].nbytes - 160, None, -1, "tri_bytes"),
             (gone_handle, new[3], None, None, -1, "destroyed plan"),
             (plan._h, new[3], None, short_ellip, -4, "EllipData shorter than its count says")]
    for handle, tris, nbytes, ellip, want_rc, text in cases:
        rc, msg, flag, cost = call(handle, tris, nbytes, ellip)
        assert rc == want_rc and text in msg and flag == -5 and (cost == -7.0).all(), (text, rc, msg)
        same_records(records(r), before, text)
        same_image(frame(pt, r, 1), img, text)
    rc, msg, flag, _ = call(plan._h, loose_only)
    assert rc == 0 and flag == 1, msg
    cost, in_place = r.move_geometry(plan, new[3])
    assert in_place is True
    got_img = frame(pt, r, 2)
    got = records(r)
    foreign.close(); plan.close(); r.close()
    fresh = context(renderer_mod, new, MC.SKY, (MC.W, MC.H))
    same_image(got_img, frame(pt, fresh, 2), "after the refusals")
    same_records(got, records(fresh), "after the refusals")
    fresh.close()


def test_read_back_is_refused_on_a_dirty_scene_and_sizes_can_be_queried(pt, renderer_mod):
    old = MC.scenes(pt)["soup3"]
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
    with pytest.raises(renderer_mod.PtError) as e:
        r.debug_scene_records("tris")
    assert e.value.code == -1 and "not built" in str(e.value)
    frame(pt, r, 1)
    n = C.c_size_t()
    L = renderer_mod.lib()
    assert L.pt_debug_scene_records(r._h, 2, None, 0, C.byref(n)) == 0 and n.value == 48 * 2 * 3       # two objects of three triangles
    small = np.zeros(4, f32)
    assert L.pt_debug_scene_records(r._h, 2, small.ctypes.data, small.nbytes, C.byref(n)) == -1 and not small.any()
    assert L.pt_debug_scene_records(r._h, 7, None, 0, C.byref(n)) == -1
    r.close()
