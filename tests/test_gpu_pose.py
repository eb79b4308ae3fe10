"""GPU: include/pt_pose.h — pt_pose_triangles against the numpy model of the rule (tests/_pose_model.py), and pt_pose_geometry against a twin
context on which move_geometry(plan, model_posed) ran: every device record array byte for byte, the frames, the host copies as later readers
see them, the moving-geometry workflow, the slow paths and the refusals.  48 x 27 or 96 x 54, a few frames.

A NaN the rule generates (inf * 0, inf - inf) equals any NaN: its sign and payload are the hardware's, and the model runs on another.  Everything
else is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _move_cases as MC
import _pose_model as PM
import _refit_cases as RC
from test_gpu_move import context, frame, records, same_image, same_records
from test_gpu_parity import _soup_obj, seeds_for

pytestmark = pytest.mark.gpu

f32 = np.float32
_CACHE = {}


def same_floats(got, want, tag):
    g, w = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    ok = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
    assert g.shape == w.shape and ok.all(), (tag, int((~ok).sum()), np.nonzero(~ok)[0][:8])


def one_soup(pt, n):
    """a complete scene of ONE object of n triangles"""
    key = ("soup", n)
    if key not in _CACHE:
        sc = pt.hostlib.Scene(); sc.addMaterial("m")
        sc.addObjectText(_soup_obj(np.random.RandomState(300 + n), n, 0.0), 0)
        _CACHE[key] = MC.complete(pt, sc.pack())
        assert _CACHE[key][3].size == 40 * n
    return _CACHE[key]


def posed(old, parts, X):
    """the scene after the pose, by the models: binding 3 by the rule, binding 10 by the refit model"""
    key = ("posed", id(old[3]), parts.tobytes(), np.ascontiguousarray(X, f32).tobytes())
    if key not in _CACHE:
        new = dict(old)
        new[3], new[10] = MC.move_of(old, PM.pose(old[3], parts, X))
        _CACHE[key] = (old[3], new)
    return _CACHE[key][1]


# ------------------------------------------------------------------------------------------------ the rule alone

@pytest.mark.parametrize("n", [2, 42, 43, 44, 255, 256, 257, 1000])
def test_pose_triangles_equals_the_model(pt, renderer_mod, n):
    """one lane per float4, 256 lanes per block: 42 triangles and four lanes of the 43rd fill a block, so 43 and 44 straddle its seam (and 255 / 256 /
    257 that of one lane per triangle).  Every third triangle holds +-0, denormals, +-inf and 3e38; the trees are the ordinary soup's."""
    b = dict(one_soup(pt, n))
    t = b[3].reshape(-1, 40).copy()
    t[::3, :24] = PM.special_triangles(len(t[::3]), seed=n).reshape(-1, 40)[:, :24]
    b[3] = t.reshape(-1)
    parts = PM.parts_mod4(n)
    r = context(renderer_mod, b, MC.SKY, (MC.W, MC.H))
    pose = r.pose_create(parts, 3)
    for seed in (5, 6):
        X = PM.matrices(3, seed)
        got = pose.triangles(X)
        same_floats(got, PM.pose(b[3], parts, X), (n, seed))
        static = np.repeat(parts < 0, 40)
        assert np.array_equal(got.view(np.uint32)[static], b[3].view(np.uint32)[static])
    X = PM.matrices(3, 7); X[0, :21] = PM.SPECIAL[np.arange(21) % PM.SPECIAL.size]; X[2, 3] = np.inf
    same_floats(pose.triangles(X), PM.pose(b[3], parts, X), (n, "special matrices"))
    none = r.pose_create(np.full(n, -1, np.int32), 0)
    assert np.array_equal(none.triangles(np.zeros(0, f32)).view(np.uint32), b[3].view(np.uint32))      # n_parts = 0: the rest pose
    none.close(); pose.close(); r.close()


@pytest.mark.parametrize("n", [43, 257])
def test_both_statements_of_the_pose_kernel_equal_the_model(pt, renderer_mod, n):
    """pt_debug_pose_time fills the scratch copy with the rest pose and runs the statement asked for, so pt_debug_pose_scratch reads that kernel's
    work: one lane per float4 (a block ends inside the 43rd triangle) and one lane per triangle (the second block starts at the 257th), the only
    place that holds k_pose_tris to the model.  The scene and the matrices are the test's above; the scratch copy holds another pose beforehand."""
    b = dict(one_soup(pt, n))
    t = b[3].reshape(-1, 40).copy()
    t[::3, :24] = PM.special_triangles(len(t[::3]), seed=n).reshape(-1, 40)[:, :24]
    b[3] = t.reshape(-1)
    parts = PM.parts_mod4(n)
    assert (parts < 0).any()
    r = context(renderer_mod, b, MC.SKY, (MC.W, MC.H))
    L = renderer_mod.lib()
    pose = r.pose_create(parts, 3)
    X = PM.matrices(3, 5)
    want = PM.pose(b[3], parts, X)
    pose.triangles(PM.matrices(3, 6))
    x = np.ascontiguousarray(X, f32).reshape(-1)
    for which in (0, 1):
        best = C.c_float(-1.0)
        assert L.pt_debug_pose_time(pose._h, x.ctypes.data, x.nbytes, which, 1, C.byref(best)) == 0, L.pt_last_error()
        assert best.value >= 0.0
        got = np.empty(n * 40, f32)
        assert L.pt_debug_pose_scratch(pose._h, got.ctypes.data, got.nbytes) == 0, L.pt_last_error()
        same_floats(got, want, (n, "statement", which))
    pose.close(); r.close()


# ------------------------------------------------------------------------------------------------ records and frames against the twin

def pose_equals_twin(pt, renderer_mod, old, tex, size, parts, n_parts, X, tag, ellip=None, want_in_place=True, **opts):
    P = PM.pose(old[3], parts, X)
    out = []
    for twin in (False, True):
        r = context(renderer_mod, old, tex, size, **opts)
        frame(pt, r, 1)
        if twin:
            plan = renderer_mod.RefitPlan(old)
            cost, in_place = r.move_geometry(plan, P, ellip)
        else:
            pose = r.pose_create(parts, n_parts)
            cost, in_place = r.pose_geometry(pose, X, ellip)
        assert in_place == want_in_place, (tag, twin)
        at_once = records(r, skip=("ellip",))
        img = frame(pt, r, 2)
        out.append((cost, at_once, img, records(r)))
        (plan if twin else pose).close(); r.close()
    (cost, at_once, img, got), (cost2, at_once2, img2, want) = out
    assert np.array_equal(cost.view(np.uint64), cost2.view(np.uint64)) and cost.size == int(old[13][0]), tag
    same_records(at_once, at_once2, (tag, "before the next render"))
    same_records(got, want, tag)
    same_image(img, img2, tag)
    return got


def soup_pose(pt, name):
    old = MC.scenes(pt)[name]
    return old, PM.parts_mod4(old[3].size // 40), PM.matrices(3)


SCENES = ["soup2", "soup128", "soup129", "soup257", "soup1000", "objects70", "leafroot", "emptyleaf"]
VARIANTS = [dict(asm_node_layout=0), dict(asm_node_layout=1), dict(bfs_nodes=3)]


@pytest.mark.parametrize("name", SCENES)
def test_records_equal_the_twin_s(pt, renderer_mod, name):
    old, parts, X = soup_pose(pt, name)
    got = pose_equals_twin(pt, renderer_mod, old, MC.SKY, (MC.W, MC.H), parts, 3, X, name)
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
    frame(pt, r, 1)
    was = records(r)
    # the pose did move something (emptyleaf's one moving triangle is in no leaf and has no normals: only its binding 3 changes)
    assert name == "emptyleaf" or not (np.array_equal(got["tris"], was["tris"]) or np.array_equal(got["shade"], was["shade"]))
    r.close()


@pytest.mark.parametrize("opts", VARIANTS, ids=["layout0", "layout1", "bfs3"])
@pytest.mark.parametrize("name", SCENES)
def test_records_equal_the_twin_s_under_the_layout_options(pt, renderer_mod, name, opts):
    old, parts, X = soup_pose(pt, name)
    pose_equals_twin(pt, renderer_mod, old, MC.SKY, (MC.W, MC.H), parts, 3, X, (name, opts), **opts)


@pytest.mark.parametrize("opts", [{}] + VARIANTS, ids=["default", "layout0", "layout1", "bfs3"])
def test_records_equal_the_twin_s_on_c6_with_64_roots(pt, renderer_mod, opts):
    wl = RC.workload(pt, "C6")
    old, tex = MC.workload_inputs(wl)
    assert int(old[13][0]) == 64
    n = old[3].size // 40
    got = pose_equals_twin(pt, renderer_mod, old, tex, (wl.W, wl.H), PM.parts_mod4(n), 3, PM.matrices(3, 9) * f32(1.0), ("C6", opts), **opts)
    assert got["roots"].size == (64 + 64) * 8


@pytest.fixture(scope="module")
def m1(pt):
    """(M1's rest pose, its buffers and textures, a part per triangle: the room static, the box, the sphere and the poster one part each, and two poses)"""
    rest = pt.scenes.m1_moving(0)
    old, tex = MC.workload_inputs(rest)
    n = old[3].size // 40
    assert n > 334
    parts = np.full(n, -1, np.int32)
    parts[n - 334:n - 322] = 0; parts[n - 322:n - 2] = 1; parts[n - 2:] = 2
    M = [[PM.rotation((0, 1, 0), 0.02 * s, (0.02 * s, 0.0, -0.01 * s)), PM.rotation((0, 1, 0), 0.03 * s), PM.rotation((1, 0, 0), 0.0, (0.015 * s, 0, 0))] for s in (2, 4)]
    return rest, old, tex, parts, [PM.records(np.array(m)) for m in M]


def test_records_equal_the_twin_s_on_m1_with_its_moved_ellipsoid(pt, renderer_mod, m1):
    rest, old, tex, parts, Xs = m1
    ellip = pt.scenes.m1_moving(4).buffers[7]
    pose_equals_twin(pt, renderer_mod, old, tex, (rest.W, rest.H), parts, 3, Xs[1], "M1", ellip=ellip)
    for opts in VARIANTS:
        pose_equals_twin(pt, renderer_mod, old, tex, (rest.W, rest.H), parts, 3, Xs[0], ("M1", opts), **opts)


def test_two_frames_equal_the_twin_s_on_the_counting_and_the_shipped_kernels(pt, renderer_mod, m1):
    rest, old, tex, parts, Xs = m1
    P = PM.pose(old[3], parts, Xs[1])
    seeds = seeds_for(pt, 1, 2)
    out = []
    for twin in (False, True):
        r = context(renderer_mod, old, tex, (rest.W, rest.H))
        frame(pt, r, 1)
        if twin:
            plan = renderer_mod.RefitPlan(old)
            assert r.move_geometry(plan, P)[1] is True
        else:
            pose = r.pose_create(parts, 3)
            assert r.pose_geometry(pose, Xs[1])[1] is True
        r.set_option("count_stats", 1)
        r.reset_frame(); r.reset_counters()
        r.render_batch(1, seeds)
        counted, cnt = r.read_frame(), r.counters()
        r.set_option("count_stats", 0)
        r.reset_frame()
        r.render_batch(1, seeds)
        out.append((counted, cnt, r.read_frame()))
        (plan if twin else pose).close(); r.close()
    same_image(out[0][0], out[1][0], "counting kernels")
    same_image(out[0][2], out[1][2], "shipped kernels")
    same_image(out[0][0], out[0][2], "shipped kernels against the counting variants")
    assert out[0][1] == out[1][1] and out[0][0][..., :3].max() > 0


def test_three_poses_end_in_the_rest_pose_s_records(pt, renderer_mod, m1):
    """two poses of one pose object, then the pose of a second one with n_parts = 0 (every triangle static), which supersedes them: the records
    and the frame are the twin's after move_geometry back to the rest pose's binding 3"""
    rest, old, tex, parts, Xs = m1
    out = []
    for twin in (False, True):
        r = context(renderer_mod, old, tex, (rest.W, rest.H))
        frame(pt, r, 1)
        seen = []
        if twin:
            plan = renderer_mod.RefitPlan(old)
            for tris in (PM.pose(old[3], parts, Xs[0]), PM.pose(old[3], parts, Xs[1]), old[3]):
                assert r.move_geometry(plan, tris)[1] is True
                frame(pt, r, 2)
                seen.append(records(r))
            plan.close()
        else:
            pose, none = r.pose_create(parts, 3), r.pose_create(np.full(parts.size, -1, np.int32), 0)
            for p, X in ((pose, Xs[0]), (pose, Xs[1]), (none, np.zeros(0, f32))):
                assert r.pose_geometry(p, X)[1] is True
                frame(pt, r, 2)
                seen.append(records(r))
        out.append((seen, frame(pt, r, 2)))
        r.close()
    for k in range(3):
        same_records(out[0][0][k], out[1][0][k], ("pose", k))
    same_image(out[0][1], out[1][1], "the rest pose again")
    assert not np.array_equal(out[0][0][0]["tris"], out[0][0][1]["tris"]) and not np.array_equal(out[0][0][1]["nodes"], out[0][0][2]["nodes"])
    fresh = context(renderer_mod, old, tex, (rest.W, rest.H))
    frame(pt, fresh, 2)
    same_records({k: v for k, v in out[0][0][2].items() if k != "nodes" and k != "nodes80" and k != "roots"},
                 {k: v for k, v in records(fresh).items() if k != "nodes" and k != "nodes80" and k != "roots"}, "the rest pose's triangles")
    fresh.close()


# ------------------------------------------------------------------------------------------------ the host copies

def fresh_records(pt, renderer_mod, b, tex, size, **opts):
    r = context(renderer_mod, b, tex, size, **opts)
    img = frame(pt, r, 2)
    out = records(r)
    r.close()
    return out, img


def test_a_rebuild_after_a_pose_reads_the_settled_copies(pt, renderer_mod):
    """an option that dirties the scene makes the next render lay it out again, from host copies the pose never wrote: they are settled first.
    The same after pt_pose_destroy; and pt_set_buffer(10) after a pose leaves binding 3 as posed."""
    old, parts, X = soup_pose(pt, "soup129")
    new = posed(old, parts, X)
    want, ref = fresh_records(pt, renderer_mod, new, MC.SKY, (MC.W, MC.H), asm_node_layout=1)
    for how in ("option", "destroy", "binding 10"):
        r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
        frame(pt, r, 1)
        pose = r.pose_create(parts, 3)
        assert r.pose_geometry(pose, X)[1] is True
        if how == "destroy":
            pose.close()
        if how == "binding 10":
            r.set_buffer(10, new[10])                             # (the refit binding 10 again: binding 3 must be the posed one underneath)
        r.set_option("asm_node_layout", 1)
        img = frame(pt, r, 2)
        same_records(records(r), want, how)
        same_image(img, ref, how)
        r.close()


# ------------------------------------------------------------------------------------------------ the moving-geometry workflow

def _workflow(pt, renderer_mod, m1, by_pose, bilinear, behind_at_the_mark, running=False):
    rest, old, tex, parts, Xs = m1
    r = context(renderer_mod, old, tex, (rest.W, rest.H))
    plan = renderer_mod.RefitPlan(old)
    pose = r.pose_create(parts, 3)
    out = []

    def move(X):
        if by_pose:
            assert r.pose_geometry(pose, X)[1] is True
        else:
            assert r.move_geometry(plan, PM.pose(old[3], parts, X))[1] is True

    first = 1
    if behind_at_the_mark:
        frame(pt, r, 1)
        move(Xs[0])                                                   # the host copies are behind when the mark is taken
    r.reset_frame()
    for X in (Xs[1], Xs[0]):
        if running:
            r.render_batch_async(first, seeds_for(pt, first, 4))      # not read: the pose finds the frame stream running
        else:
            r.render_batch(first, seeds_for(pt, first, 4))
            r.motion_mark()
        move(X)
        if running:
            out.append(r.read_frame().copy())
        else:
            out.append(r.reproject_frame_moved_bilinear() if bilinear else r.reproject_frame_moved())
            out.append(r.read_frame().copy())
        first += 4
    r.render_batch(first, seeds_for(pt, first, 1))
    out.append(r.read_frame().copy())
    pose.close(); plan.close(); r.close()
    return out


@pytest.mark.parametrize("behind", [False, True], ids=["mark-current", "mark-behind"])
@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
def test_motion_workflow_equals_the_twin_s(pt, renderer_mod, m1, bilinear, behind):
    a = _workflow(pt, renderer_mod, m1, True, bilinear, behind)
    b = _workflow(pt, renderer_mod, m1, False, bilinear, behind)
    assert len(a) == len(b) == 5
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            same_image(x, y, k)
        else:
            assert x == y and np.all(np.asarray(x) > 0), (k, x, y)


def test_a_pose_under_a_running_frame_stream_equals_the_twin(pt, renderer_mod, m1):
    a = _workflow(pt, renderer_mod, m1, True, False, False, running=True)
    b = _workflow(pt, renderer_mod, m1, False, False, False, running=True)
    assert len(a) == len(b) == 3
    for k, (x, y) in enumerate(zip(a, b)):
        same_image(x, y, k)
    assert a[2][..., 3].max() > a[1][..., 3].max() > a[0][..., 3].max() > 0      # nothing was reset: 4, 8 and 9 frames


def test_a_mark_taken_behind_serves_a_reprojection_over_current_copies(pt, renderer_mod, m1):
    """pose, mark (its records are made on the device), then pt_move_geometry, which settles: the reprojection packs on the host again and fetches
    the mark's host positions from the mark's device records"""
    rest, old, tex, parts, Xs = m1
    P = [PM.pose(old[3], parts, X) for X in Xs]
    out = []
    for twin in (False, True):
        r = context(renderer_mod, old, tex, (rest.W, rest.H))
        plan = renderer_mod.RefitPlan(old)
        pose = r.pose_create(parts, 3)
        frame(pt, r, 1)
        if twin:
            assert r.move_geometry(plan, P[0])[1] is True
        else:
            assert r.pose_geometry(pose, Xs[0])[1] is True
        r.reset_frame()
        r.render_batch(1, seeds_for(pt, 1, 4))
        r.motion_mark()
        assert r.move_geometry(plan, P[1])[1] is True
        out.append((r.reproject_frame_moved(), r.read_frame().copy()))
        pose.close(); plan.close(); r.close()
    assert out[0][0] == out[1][0] and out[0][0] > 0
    same_image(out[0][1], out[1][1], "the mark's positions fetched from the device")


# ------------------------------------------------------------------------------------------------ ordering and validity

def test_a_pose_is_stale_after_an_upload_and_move_geometry_settles_first(pt, renderer_mod):
    old, parts, X = soup_pose(pt, "soup129")
    new = posed(old, parts, X)
    tris2, data2 = MC.move_of(old, RC.perturbed(new[3], 13))
    out = []
    for twin in (False, True):
        r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
        frame(pt, r, 1)
        plan = renderer_mod.RefitPlan(old)
        pose = r.pose_create(parts, 3)
        if twin:
            assert r.move_geometry(plan, new[3])[1] is True
        else:
            assert r.pose_geometry(pose, X)[1] is True
        assert r.move_geometry(plan, tris2)[1] is True              # on a context that is behind
        img = frame(pt, r, 2)
        out.append((records(r), img))
        with pytest.raises(renderer_mod.PtError) as e:               # pt_move_geometry made the pose stale
            r.pose_geometry(pose, X)
        assert e.value.code == -4 and "the scene was uploaded since pt_pose_create" in str(e.value)
        same_records(records(r), out[-1][0], "a stale pose changes nothing")
        r.set_option("asm_node_layout", 1)                            # the host copies are the second move's
        out[-1] += (records_after(pt, r),)
        pose.close(); plan.close(); r.close()
    same_records(out[0][0], out[1][0], "move on a context that is behind")
    same_image(out[0][1], out[1][1], "move on a context that is behind")
    same_records(out[0][2], out[1][2], "the rebuild after it")
    # an upload of binding 3
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
    frame(pt, r, 1)
    pose = r.pose_create(parts, 3)
    assert r.pose_geometry(pose, X)[1] is True
    r.set_buffer(3, old[3])
    with pytest.raises(renderer_mod.PtError) as e:
        r.pose_geometry(pose, X)
    assert e.value.code == -4 and "the scene was uploaded since pt_pose_create" in str(e.value)
    again = r.pose_create(parts, 3)                                   # a new pose over the uploaded scene works
    assert r.pose_geometry(again, X)[1] is True
    frame(pt, r, 2)
    same_records(records(r), fresh_records(pt, renderer_mod, new, MC.SKY, (MC.W, MC.H))[0], "a new pose after the upload")
    r.close()


def records_after(pt, r):
    frame(pt, r, 2)
    return records(r)


# ------------------------------------------------------------------------------------------------ the slow paths

def test_slow_path_multi_stream_context(pt, renderer_mod, m1):
    """three poses in a row on one multi-stream context (X0, X1, X0 again: the call's own uploads do not make the pose stale): after each, in_place
    is False, root_cost is the refit's and the frame is a fresh multi-stream context's over the model's buffers"""
    rest, old, tex, parts, Xs = m1
    r = renderer_mod.Renderer(rest.W, rest.H, devices=[0, 0])
    r.load_workload(rest)
    frame(pt, r, 1)
    pose = r.pose_create(parts, 3)
    plan = renderer_mod.RefitPlan(old)
    seen = []
    for k in (0, 1, 0):
        new = posed(old, parts, Xs[k])
        cost, in_place = r.pose_geometry(pose, Xs[k])
        assert in_place is False, k
        assert np.array_equal(cost.view(np.uint64), plan.run(new[3])[1].view(np.uint64)), k
        assert np.array_equal(pose.triangles(Xs[k]).view(np.uint32), new[3].view(np.uint32)), k
        seen.append(frame(pt, r, 2))
    r.set_buffer(3, old[3])                                           # the caller's own upload does
    with pytest.raises(renderer_mod.PtError) as e:
        r.pose_geometry(pose, Xs[0])
    assert e.value.code == -4 and "the scene was uploaded since pt_pose_create" in str(e.value)
    pose.close(); plan.close(); r.close()
    for k in (0, 1):
        fresh = renderer_mod.Renderer(rest.W, rest.H, devices=[0, 0])
        for key, a in posed(old, parts, Xs[k]).items():
            fresh.set_buffer(key, a)
        for i, t in tex.items():
            fresh.set_texture(i, t)
        ref = frame(pt, fresh, 2)
        fresh.close()
        same_image(seen[k], ref, ("multi", k))
        if k == 0:
            same_image(seen[2], ref, ("multi", "X0 again"))
    assert not np.array_equal(seen[0], seen[1])


def test_slow_path_binding_7_with_another_material(pt, renderer_mod, m1):
    rest, old, tex, parts, Xs = m1
    e = pt.scenes.m1_moving(4).buffers[7].copy()
    assert e[0] == 1.0 and e[11] != 0.0
    e[11] = 0.0
    pose_equals_twin(pt, renderer_mod, old, tex, (rest.W, rest.H), parts, 3, Xs[1], "M1 other material", ellip=e, want_in_place=False)


# ------------------------------------------------------------------------------------------------ the refusals

def test_refusals_leave_records_image_and_settled_copies_as_they_were(pt, renderer_mod):
    old, parts, X1 = soup_pose(pt, "soup129")
    X2 = PM.matrices(3, 21)
    new1, new2 = posed(old, parts, X1), posed(old, parts, X2)
    L = renderer_mod.lib()
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H), asm_node_layout=0)
    other = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
    frame(pt, r, 1)
    pose = r.pose_create(parts, 3)
    foreign = other.pose_create(parts, 3)
    gone = r.pose_create(parts, 3)
    gone_handle = C.c_void_p(gone._h.value)
    gone.close()
    assert r.pose_geometry(pose, X1)[1] is True                      # the last accepted pose: the context is behind on it
    img = frame(pt, r, 2)
    before = records(r)
    nan = X1.copy(); nan[1, 5] = np.nan                               # part 1 is referenced
    inf = X1.copy(); inf[0, 0] = np.inf; inf[0, 1] = -np.inf          # inf * x - inf * y: a NaN wherever x and y have the same sign
    with np.errstate(all="ignore"):
        bad = PM.pose(old[3], parts, inf).reshape(-1, 40)
    assert np.isnan(bad[:, :11]).any() and not np.isnan(PM.pose(old[3], parts, X1)).any()

    def call(handle, X, nbytes=None):
        flag = C.c_int(-5)
        cost = np.full(pose.n_roots, -7.0)
        X = np.ascontiguousarray(X, f32)
        rc = L.pt_pose_geometry(r._h, handle, X.ctypes.data, X.nbytes if nbytes is None else nbytes, None, 0, cost.ctypes.data, C.byref(flag))
        return rc, L.pt_last_error().decode(), flag.value, cost

    cases = [(pose._h, nan, None, -4, "pt_pose_geometry: NaN coordinate in a referenced triangle"),
             (pose._h, inf, None, -4, "pt_pose_geometry: NaN coordinate in a referenced triangle"),
             (pose._h, X1, X1.nbytes - 4, -1, "xform_bytes != n_parts * 96"),
             (pose._h, X1, X1.nbytes + 96, -1, "xform_bytes != n_parts * 96"),
             (foreign._h, X1, None, -1, "the pose was created on another context"),
             (gone_handle, X1, None, -1, "null or destroyed pose")]
    fresh = {layout: fresh_records(pt, renderer_mod, new1, MC.SKY, (MC.W, MC.H), asm_node_layout=layout) for layout in (0, 1)}
    layout = 0
    for handle, X, nbytes, want_rc, text in cases:
        rc, msg, flag, cost = call(handle, X, nbytes)
        assert rc == want_rc and text in msg and flag == -5 and (cost == -7.0).all(), (text, rc, msg)
        same_records(records(r), before, text)
        same_image(frame(pt, r, 2), img, text)
        # what a settle delivers after THIS refusal is the last accepted pose: the rebuild an option change forces reads the settled copies
        layout = 1 - layout
        r.set_option("asm_node_layout", layout)
        got_img = frame(pt, r, 2)
        same_records(records(r), fresh[layout][0], (text, "the settled copies"))
        same_image(got_img, fresh[layout][1], (text, "the settled copies"))
        r.set_option("asm_node_layout", 0)                            # back, and behind on the accepted pose again for the next case
        layout = 0
        assert r.pose_geometry(pose, X1)[1] is True
        same_image(frame(pt, r, 2), img, (text, "the accepted pose again"))
        same_records(records(r), before, (text, "the accepted pose again"))
    # a good pose still works; a refusal after it leaves ITS copies
    assert r.pose_geometry(pose, X2)[1] is True
    rc, msg, flag, cost = call(pose._h, nan)
    assert rc == -4 and flag == -5, msg
    r.set_option("asm_node_layout", 1)
    got_img = frame(pt, r, 2)
    want, ref = fresh_records(pt, renderer_mod, new2, MC.SKY, (MC.W, MC.H), asm_node_layout=1)
    same_records(records(r), want, "a good pose after the refusals")
    same_image(got_img, ref, "a good pose after the refusals")
    foreign.close(); pose.close(); other.close(); r.close()


def test_refusals_of_a_pose_without_parts_leave_the_rest_pose(pt, renderer_mod):
    """n_parts = 0: every triangle static, the only pose is the rest pose; the context is behind on it with no matrices accepted.  A refused call
    (matrices where none are taken) changes nothing, and a settle delivers the rest pose with its refit binding 10"""
    old, parts, X = soup_pose(pt, "soup129")
    n = parts.size
    L = renderer_mod.lib()
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
    frame(pt, r, 1)
    none = r.pose_create(np.full(n, -1, np.int32), 0)
    cost, in_place = r.pose_geometry(none, np.zeros(0, f32))
    assert in_place is True
    img = frame(pt, r, 2)
    before = records(r)
    flag = C.c_int(-5)
    x = np.ascontiguousarray(X, f32)
    assert L.pt_pose_geometry(r._h, none._h, x.ctypes.data, 96, None, 0, None, C.byref(flag)) == -1 and flag.value == -5
    assert b"xform_bytes != n_parts * 96" in L.pt_last_error()
    same_records(records(r), before, "n_parts = 0")
    same_image(frame(pt, r, 2), img, "n_parts = 0")
    new = dict(old); new[3], new[10] = MC.move_of(old, old[3])
    assert np.array_equal(cost.view(np.uint64), renderer_mod.RefitPlan(old).run(old[3])[1].view(np.uint64))
    r.set_option("asm_node_layout", 1)
    got_img = frame(pt, r, 2)
    want, ref = fresh_records(pt, renderer_mod, new, MC.SKY, (MC.W, MC.H), asm_node_layout=1)
    same_records(records(r), want, "the settled rest pose")
    same_image(got_img, ref, "the settled rest pose")
    none.close(); r.close()
