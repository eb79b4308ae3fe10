"""GPU: include/pt_normals.h — the kernels against the numpy model of the rule (tests/_normals_model.py) through pt_pose_triangles and, for both
statements of the gather, through pt_debug_normals_time followed by pt_debug_pose_scratch; the chain morph -> skin -> normals against the chained
models; and pt_pose_geometry of a pose with normals against a twin context on which move_geometry(plan, model_triangles) ran: every device record
array byte for byte, the frames, root_cost, the reprojection workflow, the refusal and what it restores (records, weights AND mode), staleness, the
attach-time refusals that need a device-made pose, the multi-stream slow path, M5 against the oracle.  48 x 27 or 96 x 54, a few frames.

A NaN the pose's rule generates equals any NaN: its sign and payload are the hardware's, and the model runs on another.  Everything else is
compared bit for bit."""
import copy
import ctypes as C

import numpy as np
import pytest

import _morph_model as MM
import _move_cases as MC
import _normals_model as NM
import _pose_model as PM
import _skin_model as SM
from test_gpu_morph import make_pose, same_bits, with_specials
from test_gpu_move import context, frame, records, same_image, same_records
from test_gpu_parity import assert_same, seeds_for
from test_gpu_pose import fresh_records, one_soup, same_floats
from test_gpu_skin import scene_of, scratch

pytestmark = pytest.mark.gpu

f32 = np.float32


def attach(pose, ids, n_vertices=None, flip=False):
    assert hasattr(pose._L, "pt_normals_attach") and hasattr(pose, "normals_attach")      # never skipped: a library without the symbol fails here
    assert hasattr(pose._L, "pt_normals_mode") and hasattr(pose._L, "pt_debug_normals_time")
    pose.normals_attach(ids, n_vertices, flip)
    return pose


def both_statements(r, pose, X, want, tag):
    """pt_debug_normals_time poses into the scratch copy with the rule's normals and then runs the statement asked for: what lies there is its work"""
    x = np.ascontiguousarray(X, f32).reshape(-1)
    for which in (0, 1):
        best = C.c_float(-1.0)
        assert r._L.pt_debug_normals_time(pose._h, x.ctypes.data, x.nbytes, which, 2, C.byref(best)) == 0, r._L.pt_last_error()
        assert best.value >= 0.0
        same_floats(scratch(r, pose), want, (tag, "statement", which))


def fan_ids(n):
    """n triangles around vertex 0: one row of n corners"""
    k = np.arange(n)
    return np.stack([np.zeros(n, np.int64), 1 + k, 1 + (k + 1) % n], axis=1).astype(np.int32).reshape(-1)


# ------------------------------------------------------------------------------------------------ the kernels against the model

def _ids_of(case, n, allowed):
    if case == "one":
        return np.array([0, 1, 2], np.int32)
    if case == "edge":
        return np.array([0, 1, 2, 2, 1, 3], np.int32)                    # two triangles sharing an edge
    if case.startswith("count"):
        return NM.ids_counted(n, int(case[5:]))
    if case == "fan":
        return fan_ids(n)
    return NM.random_ids(allowed, max(n // 3, 2), seed=n, minus=0.25, n_tris=n)


KERNEL_CASES = [(1, "all", "one", False), (2, "all", "edge", True), (300, "all", "count255", False), (300, "all", "count256", True), (300, "all", "count257", False),
                (300, "all", "fan", False), (257, "mod4", "random", True), (1000, "skin", "random", False)]


@pytest.mark.parametrize("n, kind, case, flip", KERNEL_CASES, ids=[f"{n}-{kind}-{case}" for n, kind, case, _ in KERNEL_CASES])
def test_the_kernels_equal_the_model(pt, renderer_mod, n, kind, case, flip):
    """One lane per listed triangle, per non-empty vertex or per corner, 256 lanes per block: 255, 256 and 257 listed triangles and vertices end
    before, at and after a block's last lane.  Every third triangle holds +-0, denormals, +-inf and 3e38, so some vertices take the fallback;
    -1 corners are mixed in; mod4 puts static triangles between moved ones, the skin static corners inside moved triangles."""
    special = n > 2 and case != "fan"                                      # (the fan's long row is summed over ordinary face vectors)
    b = with_specials(scene_of(pt, n), seed=n + len(case)) if special else scene_of(pt, n)
    r = context(renderer_mod, b, MC.SKY, (MC.W, MC.H))
    pose, allowed, model, X = make_pose(r, kind, n, seed=n)
    plain = make_pose(r, kind, n, seed=n)[0]                             # the same pose without normals, on the same context
    ids = _ids_of(case, n, allowed)
    listed, verts, start, _, _ = NM.rows(ids)
    if case.startswith("count"):
        assert listed.size == verts.size == int(case[5:]) and len(set(np.diff(start).tolist())) > 1
    if case == "fan":
        assert np.diff(start).max() == 300
    attach(pose, ids, flip=flip)
    ruled = plain.triangles(X)
    by_model = model(b[3])
    same_floats(ruled, by_model, (case, "the pose alone"))
    want, fell = NM.smooth(by_model, ids, flip=flip, want_fallbacks=True)
    got = pose.triangles(X)
    same_floats(got, want, (n, kind, case))
    both_statements(r, pose, X, want, (n, kind, case))
    # what is static or -1 keeps the bits of the pose alone; every fallback the model takes was taken
    g, p = got.view(np.uint32).reshape(-1, 40), ruled.view(np.uint32).reshape(-1, 40)
    keep = np.ones((n, 40), bool)
    q = np.nonzero(ids >= 0)[0]
    for j in range(3):
        keep[q // 3, 12 + 4 * (q % 3) + j] = False
    nan = np.isnan(got.reshape(-1, 40)) & np.isnan(ruled.reshape(-1, 40))
    assert ((g == p) | nan)[keep].all()
    for v in fell:
        for c in np.nonzero(ids == v)[0]:
            k, cc = divmod(int(c), 3)
            assert ((g[k, 12 + 4 * cc:15 + 4 * cc] == p[k, 12 + 4 * cc:15 + 4 * cc]) | nan[k, 12 + 4 * cc:15 + 4 * cc]).all(), (case, v)
    if special:
        assert 0 < fell.size < verts.size, (fell.size, verts.size)      # both branches ran
    done = np.setdiff1d(verts, fell)
    for v in done[:200]:                                                  # a recomputed normal: finite, one per vertex
        c = np.nonzero(ids == v)[0]
        nrm = np.stack([got.reshape(-1, 40)[c // 3, 12 + 4 * (c % 3) + j] for j in range(3)], axis=1)
        assert np.isfinite(nrm).all() and (nrm.view(np.uint32) == nrm.view(np.uint32)[0]).all()
    if done.size:
        assert not np.array_equal(g, p)
    pose.normals_mode(0)
    same_bits(pose.triangles(X), ruled, (case, "mode 0: the pose without the attach"))
    pose.normals_mode(1)
    same_floats(pose.triangles(X), want, (case, "mode 1 again"))
    same_bits(plain.triangles(X), ruled, "the pose beside it is untouched")
    plain.close(); pose.close(); r.close()


# ------------------------------------------------------------------------------------------------ the chain

def test_pose_triangles_equals_morph_then_skin_then_normals(pt, renderer_mod):
    n = 257
    b = with_specials(one_soup(pt, n), seed=11)
    r = context(renderer_mod, b, MC.SKY, (MC.W, MC.H))
    pose, allowed, model, X = make_pose(r, "skin", n, seed=3)
    plain = make_pose(r, "skin", n, seed=3)[0]
    targets, _ = MM.random_targets(allowed, 300, 5, seed=8)
    ids = NM.random_ids(allowed, 90, seed=2, n_tris=n)
    pose.morph_attach(targets); plain.morph_attach(targets)
    attach(pose, ids)
    for w in (MM.special_weights(5, 1), np.zeros(5, f32), np.array([2.0, -0.75, 0.0, 1.0, 1e-39], f32)):
        pose.morph_weights(w); plain.morph_weights(w)
        ruled = model(MM.morph(b[3], targets, w))
        same_floats(pose.triangles(X), NM.smooth(ruled, ids), ("chain", w[0]))
        both_statements(r, pose, X, NM.smooth(ruled, ids), ("chain", w[0]))
        pose.normals_mode(0)
        same_bits(pose.triangles(X), plain.triangles(X), "mode 0 equals the plain pose on the same context")
        pose.normals_mode(1)
    plain.close(); pose.close(); r.close()


# ------------------------------------------------------------------------------------------------ records and frames against the twin

@pytest.fixture(scope="module")
def m5(pt):
    """(M5's rest workload, its buffers and textures, the skin tables, the targets, the ids, per step (records, weights))"""
    rest, bone, weight, targets, X, w, ids, nv = pt.scenes.m5_rippling(1)
    old, tex = MC.workload_inputs(rest)
    steps = [(X, w)] + [pt.scenes.m5_rippling(s)[4:6] for s in (3, 7)]
    return rest, old, tex, bone, weight, targets, ids, nv, steps


@pytest.fixture(scope="module")
def soup(pt):
    """(soup129, a skin over it, targets and ids on the corners it moves, records, weights)"""
    old = MC.scenes(pt)["soup129"]
    n = old[3].size // 40
    bone, weight = SM.random_skin(n, 3, seed=41)
    moved = MM.moved_corners(n, bone=bone)
    targets, _ = MM.random_targets(moved, 200, 4, seed=6, scale=0.2)
    ids = NM.random_ids(moved, 60, seed=5, n_tris=n)
    return old, bone, weight, targets, ids, PM.matrices(3), np.array([0.8, -0.5, 1e-39, 1.5], f32)


def normals_equal_twin(pt, renderer_mod, old, tex, size, create, X, P, tag, **opts):
    out = []
    for twin in (False, True):
        r = context(renderer_mod, old, tex, size, **opts)
        frame(pt, r, 1)
        if twin:
            plan = renderer_mod.RefitPlan(old)
            cost, in_place = r.move_geometry(plan, P)
        else:
            pose = create(r)
            cost, in_place = r.pose_geometry(pose, X)
        assert in_place is True, (tag, twin)
        at_once = records(r, skip=("ellip",))
        img = frame(pt, r, 2)
        out.append((cost, at_once, img, records(r)))
        (plan if twin else pose).close(); r.close()
    (cost, at_once, img, got), (cost2, at_once2, img2, want) = out
    assert np.array_equal(cost.view(np.uint64), cost2.view(np.uint64)) and cost.size == int(old[13][0]), tag      # root_cost
    same_records(at_once, at_once2, (tag, "before the next render"))
    same_records(got, want, tag)
    same_image(img, img2, tag)


@pytest.mark.parametrize("opts", [{}, dict(bfs_nodes=3)], ids=["default", "bfs3"])
def test_records_equal_the_twin_s_on_a_soup(pt, renderer_mod, soup, opts):
    old, bone, weight, targets, ids, X, w = soup
    P = NM.morph_skin_smooth(old[3], targets, w, bone, weight, X, ids, flip=True)
    assert not np.isnan(P).any() and not np.array_equal(P, MM.morph_skin(old[3], targets, w, bone, weight, X))      # the step did change normals

    def create(r):
        pose = r.skin_create(bone, weight, 3)
        pose.morph_attach(targets); pose.morph_weights(w)
        return attach(pose, ids, flip=True)
    normals_equal_twin(pt, renderer_mod, old, MC.SKY, (MC.W, MC.H), create, X, P, ("soup129", opts), **opts)


def test_records_equal_the_twin_s_on_a_soup_under_a_part_pose(pt, renderer_mod, soup):
    old, _, _, _, _, X, _ = soup
    n = old[3].size // 40
    parts = PM.parts_mod4(n)
    ids = NM.random_ids(MM.moved_corners(n, tri_part=parts), 50, seed=9, n_tris=n)
    P = NM.pose_smooth(old[3], parts, X, ids)
    normals_equal_twin(pt, renderer_mod, old, MC.SKY, (MC.W, MC.H), lambda r: attach(r.pose_create(parts, 3), ids), X, P, "soup129 parts")


def test_records_equal_the_twin_s_on_m5(pt, renderer_mod, m5):
    rest, old, tex, bone, weight, targets, ids, nv, steps = m5
    X, w = steps[1]
    P = NM.morph_skin_smooth(old[3], targets, w, bone, weight, X, ids)
    carried = MM.morph_skin(old[3], targets, w, bone, weight, X)
    assert not np.array_equal(P, carried) and np.array_equal(P.reshape(-1, 40)[:, :12], carried.reshape(-1, 40)[:, :12])      # other normals, the same vertices

    def create(r):
        pose = r.skin_create(bone, weight, 5)
        pose.morph_attach(targets); pose.morph_weights(w)
        return attach(pose, ids, nv)
    normals_equal_twin(pt, renderer_mod, old, tex, (rest.W, rest.H), create, X, P, "M5")


def test_m5_at_two_steps_equals_the_oracle_on_the_model_s_triangles(pt, oracle, renderer_mod, m5):
    """two steps on one context, two frames each: the counting kernels against the oracle on the model's triangles, image and counters"""
    rest, old, tex, bone, weight, targets, ids, nv, steps = m5
    seeds = seeds_for(pt, 1, 2)
    r = context(renderer_mod, old, tex, (rest.W, rest.H))
    r.set_option("count_stats", 1)
    frame(pt, r, 1)
    pose = r.skin_create(bone, weight, 5)
    pose.morph_attach(targets)
    attach(pose, ids, nv)
    for X, w in steps[1:]:
        P = NM.morph_skin_smooth(old[3], targets, w, bone, weight, X, ids)
        pose.morph_weights(w)
        r.pose_geometry(pose, X)
        r.reset_frame(); r.reset_counters()
        r.render_batch(1, seeds)
        got, cnt = r.read_frame(), r.counters()
        wl = copy.copy(rest)
        wl.buffers = dict(rest.buffers)
        wl.buffers[3], wl.buffers[10] = MC.move_of(old, P)
        ref, ocnt = oracle.render_frames(oracle.Scene.from_workload(wl), rest.W, rest.H, 1, 2, seeds, nthreads=8)
        assert_same(got, ref, cnt, dict(zip(oracle.COUNTERS, [int(x) for x in ocnt])))
        assert got[..., :3].max() > 0
    pose.close(); r.close()


# ------------------------------------------------------------------------------------------------ the moving-geometry workflow

def _workflow(pt, renderer_mod, m5, by_pose, behind_at_the_mark):
    """mark -> pose with normals -> reproject_frame_moved -> one frame"""
    rest, old, tex, bone, weight, targets, ids, nv, steps = m5
    r = context(renderer_mod, old, tex, (rest.W, rest.H))
    plan = renderer_mod.RefitPlan(old)
    pose = r.skin_create(bone, weight, 5)
    pose.morph_attach(targets)
    attach(pose, ids, nv)

    def move(X, w):
        if by_pose:
            pose.morph_weights(w)
            assert r.pose_geometry(pose, X)[1] is True
        else:
            assert r.move_geometry(plan, NM.morph_skin_smooth(old[3], targets, w, bone, weight, X, ids))[1] is True

    if behind_at_the_mark:
        frame(pt, r, 1)
        move(*steps[0])                                                   # the host copies are behind when the mark is taken
    r.reset_frame()
    r.render_batch(1, seeds_for(pt, 1, 4))
    r.motion_mark()
    move(*steps[1])
    kept = r.reproject_frame_moved()
    carried = r.read_frame().copy()
    r.render_batch(5, seeds_for(pt, 5, 1))
    img = r.read_frame().copy()
    pose.close(); plan.close(); r.close()
    return kept, carried, img


@pytest.mark.parametrize("behind", [False, True], ids=["mark-current", "mark-behind"])
def test_reprojection_workflow_equals_the_twin_s(pt, renderer_mod, m5, behind):
    a = _workflow(pt, renderer_mod, m5, True, behind)
    b = _workflow(pt, renderer_mod, m5, False, behind)
    assert a[0] == b[0] and np.all(np.asarray(a[0]) > 0), (a[0], b[0])      # the kept-pixel count
    same_image(a[1], b[1], "the reprojected image")
    same_image(a[2], b[2], "one frame on top")


# ------------------------------------------------------------------------------------------------ refusal and restore

def test_a_refusal_restores_the_last_accepted_records_weights_and_mode(pt, renderer_mod, soup):
    old, bone, weight, targets, ids, X, w = soup
    L = renderer_mod.lib()
    inf = X.copy(); inf[0, 0] = np.inf; inf[0, 1] = -np.inf               # inf * x - inf * y: a NaN wherever x and y have the same sign
    P1 = NM.morph_skin_smooth(old[3], targets, w, bone, weight, X, ids)
    assert not np.isnan(P1).any()
    new1 = dict(old)
    new1[3], new1[10] = MC.move_of(old, P1)
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H), asm_node_layout=0)
    frame(pt, r, 1)
    pose = r.skin_create(bone, weight, 3)
    pose.morph_attach(targets); pose.morph_weights(w)
    attach(pose, ids)
    assert r.pose_geometry(pose, X)[1] is True                           # accepted: (X, w, mode 1)
    img = frame(pt, r, 2)
    before = records(r)
    pose.normals_mode(0)                                                  # a host-side store: nothing of the context changes ...
    pose.morph_weights(np.zeros(4, f32))
    same_records(records(r), before, "after the stores")
    flag = C.c_int(-5)
    cost = np.full(pose.n_roots, -7.0)
    x = np.ascontiguousarray(inf, f32)
    rc = L.pt_pose_geometry(r._h, pose._h, x.ctypes.data, x.nbytes, None, 0, cost.ctypes.data, C.byref(flag))
    assert rc == -4 and L.pt_last_error().decode() == "pt_pose_geometry: NaN coordinate in a referenced triangle"      # PT_ERR_SCENE
    assert flag.value == -5 and (cost == -7.0).all()
    same_records(records(r), before, "refused")
    same_image(frame(pt, r, 2), img, "refused")
    r.set_option("asm_node_layout", 1)                                    # a rebuild: the settled copies are the last accepted triple's, mode 1 included
    got_img = frame(pt, r, 2)
    want, ref = fresh_records(pt, renderer_mod, new1, MC.SKY, (MC.W, MC.H), asm_node_layout=1)
    same_records(records(r), want, "the settled copies")
    same_image(got_img, ref, "the settled copies")
    assert r.pose_geometry(pose, X)[1] is True                           # and the pose is still usable: mode 0, weights 0 as stored
    new2 = dict(old)
    new2[3], new2[10] = MC.move_of(old, SM.skin(old[3], bone, weight, X))
    got_img = frame(pt, r, 2)
    want, ref = fresh_records(pt, renderer_mod, new2, MC.SKY, (MC.W, MC.H), asm_node_layout=1)
    same_records(records(r), want, "mode 0 after the refusal")
    same_image(got_img, ref, "mode 0 after the refusal")
    pose.close(); r.close()


# ------------------------------------------------------------------------------------------------ staleness, a second attach, attach-time refusals

def test_staleness_a_second_attach_and_the_refusals_that_need_a_pose(pt, renderer_mod, soup):
    old, bone, weight, targets, ids, X, w = soup
    n = old[3].size // 40
    PtError = renderer_mod.PtError
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
    frame(pt, r, 1)

    def refused(call, code, text):
        with pytest.raises(PtError) as e:
            call()
        assert e.value.code == code and text in str(e.value), str(e.value)

    none_ids = np.full(3 * n, -1, np.int32)

    def one(q, g=0):
        a = none_ids.copy(); a[q] = g
        return a

    skin = r.skin_create(bone, weight, 3)
    q_static = int(np.nonzero(bone.reshape(-1, 4)[:, 0] < 0)[0][0])
    q_moved = int(MM.moved_corners(n, bone=bone)[0])
    refused(lambda: skin.normals_attach(one(q_static), 1), -1, "pt_normals_attach: an id >= 0 at a corner that the pose's rule leaves static")
    parts = PM.parts_mod4(n)
    part = r.pose_create(parts, 3)
    refused(lambda: part.normals_attach(one(0), 1), -1, "pt_normals_attach: an id >= 0 at a corner that the pose's rule leaves static")      # triangle 0: part -1
    refused(lambda: part.normals_attach(one(3, 1), 1), -1, "pt_normals_attach: an id outside [-1, n_vertices)")
    refused(lambda: part.normals_attach(one(3), 3 * n + 1), -1, "pt_normals_attach: n_vertices outside [0, 3 * n_tris]")
    refused(lambda: part.normals_attach(none_ids[:-3], 0), -1, "pt_normals_attach: vertex_bytes != n_tris * 12")
    two = one(3); two[4] = 0
    refused(lambda: part.normals_attach(two, 1), -1, "pt_normals_attach: the same id >= 0 at two corners of one triangle")
    assert part._L.pt_normals_attach(part._h, two.ctypes.data, two.nbytes, 1, 2) == -1
    assert b"a bit of flags other than PT_NORMALS_FLIP" in part._L.pt_last_error()
    refused(lambda: part.normals_mode(1), -1, "pt_normals_mode: the pose has no normals attached")      # a refused attach attached nothing
    nothing = r.pose_create(np.full(n, -1, np.int32), 0)
    refused(lambda: nothing.normals_attach(one(0), 1), -1, "pt_normals_attach: an id >= 0 at a corner that the pose's rule leaves static")      # n_parts == 0
    attach(nothing, none_ids, 0)                                          # ... and no id: accepted
    same_bits(nothing.triangles(np.zeros(0, f32)), old[3], "n_parts = 0, null xforms: the rest pose stays the rest pose")
    # a second attach; the mode's own refusals
    attach(skin, ids)
    refused(lambda: skin.normals_attach(ids), -1, "pt_normals_attach: the pose has normals attached already")
    refused(lambda: skin.normals_mode(2), -1, "pt_normals_mode: on must be 0 or 1")
    refused(lambda: skin.normals_mode(-1), -1, "pt_normals_mode: on must be 0 or 1")
    best = C.c_float(-1.0)
    x = np.ascontiguousarray(X, f32).reshape(-1)
    assert r._L.pt_debug_normals_time(part._h, x.ctypes.data, x.nbytes, 0, 1, C.byref(best)) == -1 and best.value == -1.0      # no normals
    assert r._L.pt_debug_normals_time(skin._h, x.ctypes.data, x.nbytes, 2, 1, C.byref(best)) == -1 and best.value == -1.0      # no such statement
    assert r.pose_geometry(skin, X)[1] is True
    # stale after an upload of binding 3
    r.set_buffer(3, old[3])
    refused(lambda: r.pose_geometry(skin, X), -4, "the scene was uploaded since pt_pose_create")
    refused(lambda: part.normals_attach(one(3), 1), -4, "the scene was uploaded since pt_pose_create")
    skin.normals_mode(0); skin.normals_mode(1)                            # a host-side store: a stale pose takes it
    again = attach(r.skin_create(bone, weight, 3), ids)                   # a new pose with normals over the uploaded scene works
    assert r.pose_geometry(again, X)[1] is True
    frame(pt, r, 2)
    new = dict(old)
    new[3], new[10] = MC.move_of(old, NM.skin_smooth(old[3], bone, weight, X, ids))
    same_records(records(r), fresh_records(pt, renderer_mod, new, MC.SKY, (MC.W, MC.H))[0], "a new pose with normals after the upload")
    r.close()


# ------------------------------------------------------------------------------------------------ the slow path

def test_slow_path_multi_stream_context(pt, renderer_mod, m5):
    rest, old, tex, bone, weight, targets, ids, nv, steps = m5
    X, w = steps[1]
    new = dict(old)
    new[3], new[10] = MC.move_of(old, NM.morph_skin_smooth(old[3], targets, w, bone, weight, X, ids))
    r = renderer_mod.Renderer(rest.W, rest.H, devices=[0, 0])
    r.load_workload(rest)
    frame(pt, r, 1)
    pose = r.skin_create(bone, weight, 5)
    pose.morph_attach(targets); pose.morph_weights(w)
    attach(pose, ids, nv)
    plan = renderer_mod.RefitPlan(old)
    cost, in_place = r.pose_geometry(pose, X)
    assert in_place is False
    assert np.array_equal(cost.view(np.uint64), plan.run(new[3])[1].view(np.uint64))
    same_floats(pose.triangles(X), new[3], "multi")
    img = frame(pt, r, 2)
    pose.close(); plan.close(); r.close()
    fresh = renderer_mod.Renderer(rest.W, rest.H, devices=[0, 0])
    for key, a in new.items():
        fresh.set_buffer(key, a)
    for i, t in tex.items():
        fresh.set_texture(i, t)
    ref = frame(pt, fresh, 2)
    fresh.close()
    same_image(img, ref, "multi")
