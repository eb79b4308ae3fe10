"""GPU: include/pt_skin_dq.h — pt_pose_triangles of a DQ pose against the numpy model of the rule (tests/_skin_dq_model.py), the two timed launches
through pt_debug_skin_dq_time, and pt_pose_geometry of a DQ pose against a twin context on which move_geometry(plan, model_posed) ran: every
device record array byte for byte, the frames, root_cost, the oracle, the chain with a morph ahead and recomputed normals behind, the
reprojection workflow, the refusal of a zero-length blend and what it restores, staleness, the multi-stream slow path, the debug timers'
refusals.  48 x 27 or 96 x 54, a few frames; the shapes are the smallest at which a kernel can go wrong (one lane per corner, 256 per block:
85 triangles are 255 lanes, 86 are 258; one lane per record: 255, 256, 257 records; the largest table, 65536).

A NaN the rule generates equals any NaN: its sign and payload are the hardware's, and the model runs on another.  Everything else is compared bit
for bit."""
import copy
import ctypes as C

import numpy as np
import pytest

import _morph_model as MM
import _move_cases as MC
import _normals_model as NM
import _pose_model as PM
import _skin_dq_model as DM
import _skin_model as SM
from test_gpu_move import context, frame, records, same_image, same_records
from test_gpu_parity import assert_same, seeds_for
from test_gpu_pose import fresh_records, one_soup, same_floats
from test_gpu_skin import scene_of, scratch

pytestmark = pytest.mark.gpu

f32 = np.float32
_CACHE = {}
NAN_TEXT = "pt_pose_geometry: NaN coordinate in a referenced triangle"


def dq_create(r, bone, weight, n_parts):
    assert hasattr(r._L, "pt_skin_dq_create") and hasattr(r, "skin_create")      # never skipped: a library without the symbol fails here
    pose = r.skin_create(bone, weight, n_parts, blend="dq")
    assert pose.blend == "dq"
    return pose


def timed(r, pose, X, want, tag):
    """pt_debug_skin_dq_time fills the scratch copy with the rest pose and then runs the two launches: what lies there is theirs"""
    x = np.ascontiguousarray(X, f32).reshape(-1)
    best = C.c_float(-1.0)
    assert r._L.pt_debug_skin_dq_time(pose._h, x.ctypes.data, x.nbytes, 2, C.byref(best)) == 0, r._L.pt_last_error()
    assert best.value >= 0.0
    same_floats(scratch(r, pose), want, (tag, "timed launches"))


def soup_records(seed):
    """two records per conversion branch, then four rigid ones with angles in [0, 2 pi)"""
    return np.concatenate([DM.branch_records(seed), DM.rigid_records(4, seed)])


def posed(old, bone, weight, X):
    """the scene after the pose, by the models: binding 3 by the rule, binding 10 by the refit model"""
    key = ("posed", id(old[3]), bone.tobytes(), weight.tobytes(), np.ascontiguousarray(X, f32).tobytes())
    if key not in _CACHE:
        new = dict(old)
        new[3], new[10] = MC.move_of(old, DM.skin_dq(old[3], bone, weight, X))
        _CACHE[key] = (old[3], new)
    return _CACHE[key][1]


# ------------------------------------------------------------------------------------------------ the rule alone

@pytest.mark.parametrize("n", [1, 2, 42, 43, 44, 85, 86, 255, 256, 257, 1000])
def test_dq_triangles_equals_the_model(pt, renderer_mod, n):
    """Every third triangle holds +-0, denormals, +-inf and 3e38.  Two tables per size: 0-4 slots per corner mixed (static corners inside moving
    triangles), and one slot count for every moving corner (1 + n % 4); weights in [-0.5, 1.5], NaN in the empty slots; twelve bones that take all
    four conversion branches, and blends that take the flip (from two triangles on)."""
    b = dict(scene_of(pt, n))
    t = b[3].reshape(-1, 40).copy()
    t[::3, :24] = PM.special_triangles(len(t[::3]), seed=n).reshape(-1, 40)[:, :24]
    b[3] = t.reshape(-1)
    r = context(renderer_mod, b, MC.SKY, (MC.W, MC.H))
    slots_seen, flips = set(), 0
    for slots in (None, 1 + n % 4):
        bone, weight = DM.random_skin(n, 12, seed=n, slots=slots)
        pose = dq_create(r, bone, weight, 12)
        static = np.repeat(bone.reshape(-1, 4)[:, 0] < 0, 4).reshape(-1, 3, 4)      # per triangle, per corner: its float4 (vertex, and normal 12 on)
        keep = np.zeros((n, 40), bool); keep[:, :12] = static.reshape(n, 12); keep[:, 12:24] = static.reshape(n, 12); keep[:, 24:] = True
        for seed in (5, 6):
            X = soup_records(seed)
            info = {}
            want = DM.skin_dq(b[3], bone, weight, X, info)
            got = pose.triangles(X)
            same_floats(got, want, (n, slots, seed))
            assert np.array_equal(got.view(np.uint32)[keep.reshape(-1)], b[3].view(np.uint32)[keep.reshape(-1)])      # static corners: the rest pose's bits
            assert (np.bincount(info["branch"], minlength=4) > 0).all()
            flips += int(info["flips"].sum())
        timed(r, pose, X, want, (n, slots))
        slots_seen |= set((bone.reshape(-1, 4) >= 0).sum(axis=1).tolist())
        assert np.isnan(weight[bone < 0]).all()
        pose.close()
    assert flips > 0 or n <= 2
    assert n < 42 or slots_seen == {0, 1, 2, 3, 4}
    none = dq_create(r, *SM.random_skin(n, 0), 0)
    assert np.array_equal(none.triangles(np.zeros(0, f32)).view(np.uint32), b[3].view(np.uint32))      # n_parts = 0: the rest pose
    none.close(); r.close()


@pytest.mark.parametrize("n_parts", [1, 255, 256, 257, 65536])
def test_dq_triangles_over_tables_of_1_to_65536_records(pt, renderer_mod, n_parts):
    """k_dq_records at its block edges and at the largest table; the last record is used"""
    n = 257
    b = one_soup(pt, n)
    bone, weight = DM.dirichlet_skin(3 * n, n_parts, seed=n_parts % 97, static=0.1)
    bone[np.nonzero(bone >= 0)[0][0]] = n_parts - 1
    assert bone.max() == n_parts - 1
    X = DM.many_rigid_records(n_parts, seed=n_parts % 89)
    r = context(renderer_mod, b, MC.SKY, (MC.W, MC.H))
    pose = dq_create(r, bone, weight, n_parts)
    want = DM.skin_dq(b[3], bone, weight, X)
    assert not np.isnan(want).any()
    same_floats(pose.triangles(X), want, n_parts)
    timed(r, pose, X, want, n_parts)
    pose.close(); r.close()


# ------------------------------------------------------------------------------------------------ records and frames against the twin

def dq_equals_twin(pt, renderer_mod, old, tex, size, bone, weight, n_parts, X, tag, **opts):
    P = DM.skin_dq(old[3], bone, weight, X)
    assert not np.isnan(P).any()
    out = []
    for twin in (False, True):
        r = context(renderer_mod, old, tex, size, **opts)
        frame(pt, r, 1)
        if twin:
            plan = renderer_mod.RefitPlan(old)
            cost, in_place = r.move_geometry(plan, P)
        else:
            pose = dq_create(r, bone, weight, n_parts)
            cost, in_place = r.pose_geometry(pose, X)
        out.append((cost, in_place, records(r, skip=("ellip",)), frame(pt, r, 2), records(r)))
        (plan if twin else pose).close(); r.close()
    (cost, flag, at_once, img, got), (cost2, flag2, at_once2, img2, want) = out
    assert flag is True and flag2 is True, (tag, flag, flag2)                # the in_place flag, and equal
    assert np.array_equal(cost.view(np.uint64), cost2.view(np.uint64)) and cost.size == int(old[13][0]), tag      # root_cost
    same_records(at_once, at_once2, (tag, "before the next render"))
    same_records(got, want, tag)
    same_image(img, img2, tag)
    return got


@pytest.fixture(scope="module")
def soup(pt):
    """(soup129, tables with weights that sum to 1 and a fifth of the corners static, twelve records)"""
    old = MC.scenes(pt)["soup129"]
    bone, weight = DM.dirichlet_skin(3 * (old[3].size // 40), 12, seed=41, static=0.2)
    return old, bone, weight, soup_records(5)


@pytest.fixture(scope="module")
def m6(pt):
    """(M6's rest workload, its buffers and textures, the two tables, the records of steps 1 and 3)"""
    rest, bone, weight, X1 = pt.scenes.m6_twisting(1)
    old, tex = MC.workload_inputs(rest)
    return rest, old, tex, bone, weight, [X1, pt.scenes.m6_twisting(3)[3]]


@pytest.mark.parametrize("opts", [{}, dict(bfs_nodes=3)], ids=["default", "bfs3"])
def test_records_equal_the_twin_s_on_a_soup(pt, renderer_mod, soup, opts):
    old, bone, weight, X = soup
    got = dq_equals_twin(pt, renderer_mod, old, MC.SKY, (MC.W, MC.H), bone, weight, 12, X, ("soup129", opts), **opts)
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H), **opts)
    frame(pt, r, 1)
    was = records(r)
    assert not (np.array_equal(got["tris"], was["tris"]) or np.array_equal(got["shade"], was["shade"]))      # the pose did move something
    r.close()


@pytest.mark.parametrize("opts", [{}, dict(bfs_nodes=3)], ids=["default", "bfs3"])
def test_records_equal_the_twin_s_on_m6(pt, renderer_mod, m6, opts):
    rest, old, tex, bone, weight, Xs = m6
    dq_equals_twin(pt, renderer_mod, old, tex, (rest.W, rest.H), bone, weight, 5, Xs[1], ("M6", opts), **opts)


def test_two_frames_of_m6_equal_the_twin_s_and_the_oracle_s(pt, oracle, renderer_mod, m6):
    """M6 at step 3, two frames: the counting and the shipped kernels against the twin and against the oracle on the model's triangles"""
    rest, old, tex, bone, weight, Xs = m6
    P = DM.skin_dq(old[3], bone, weight, Xs[1])
    seeds = seeds_for(pt, 1, 2)
    out = []
    for twin in (False, True):
        r = context(renderer_mod, old, tex, (rest.W, rest.H))
        frame(pt, r, 1)
        if twin:
            plan = renderer_mod.RefitPlan(old)
            assert r.move_geometry(plan, P)[1] is True
        else:
            pose = dq_create(r, bone, weight, 5)
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
    wl = copy.copy(rest)
    wl.buffers = dict(rest.buffers)
    wl.buffers[3], wl.buffers[10] = MC.move_of(old, P)
    ref, ocnt = oracle.render_frames(oracle.Scene.from_workload(wl), rest.W, rest.H, 1, 2, seeds, nthreads=8)
    assert_same(out[0][0], ref, out[0][1], dict(zip(oracle.COUNTERS, [int(x) for x in ocnt])))
    same = (out[0][2] == ref) | (np.isnan(out[0][2]) & np.isnan(ref))
    assert same.all(), "shipped kernels against the oracle"


# ------------------------------------------------------------------------------------------------ the chain: morph ahead, normals behind

def test_m6_chained_equals_morph_then_dq_skin_then_normals(pt, renderer_mod, m6):
    """M4's targets ahead of, and M5's weld behind, a DQ skin of M6's tube"""
    rest, old, tex, bone, weight, Xs = m6
    _, _, _, targets, _, w4, ids, nv = pt.scenes.m5_rippling(3)
    r = context(renderer_mod, old, tex, (rest.W, rest.H))
    pose, plain = dq_create(r, bone, weight, 5), dq_create(r, bone, weight, 5)
    pose.morph_attach(targets)
    pose.normals_attach(ids, nv)
    X = Xs[1]
    assert (w4 != 0).any()
    for w in (w4, np.zeros(len(targets), f32)):
        pose.morph_weights(w)
        ruled = DM.skin_dq(MM.morph(old[3], targets, w), bone, weight, X)
        want = NM.smooth(ruled, ids)
        assert not np.array_equal(want, ruled)
        same_floats(pose.triangles(X), want, ("chain", float(w[0])))
        pose.normals_mode(0)
        same_floats(pose.triangles(X), ruled, ("chain, the rule's normals", float(w[0])))
        pose.normals_mode(1)
    pose.normals_mode(0)                                                  # every weight zero and mode 0: the plain DQ pose, bit for bit
    assert np.array_equal(pose.triangles(X).view(np.uint32), plain.triangles(X).view(np.uint32))
    pose.normals_mode(1)
    pose.morph_weights(w4)                                                # and the chain through pt_pose_geometry leaves what the twin's move leaves
    P = NM.smooth(DM.skin_dq(MM.morph(old[3], targets, w4), bone, weight, X), ids)
    frame(pt, r, 1)
    cost, in_place = r.pose_geometry(pose, X)
    assert in_place is True
    got = records(r)
    plain.close(); pose.close(); r.close()
    r = context(renderer_mod, old, tex, (rest.W, rest.H))
    frame(pt, r, 1)
    plan = renderer_mod.RefitPlan(old)
    cost2, in_place = r.move_geometry(plan, P)
    assert in_place is True and np.array_equal(cost.view(np.uint64), cost2.view(np.uint64))
    same_records(got, records(r), "chain")
    plan.close(); r.close()


# ------------------------------------------------------------------------------------------------ the moving-geometry workflow

def _workflow(pt, renderer_mod, m6, by_pose, behind_at_the_mark):
    """mark -> DQ pose -> reproject_frame_moved -> frames"""
    rest, old, tex, bone, weight, Xs = m6
    r = context(renderer_mod, old, tex, (rest.W, rest.H))
    plan = renderer_mod.RefitPlan(old)
    pose = dq_create(r, bone, weight, 5)

    def move(X):
        if by_pose:
            assert r.pose_geometry(pose, X)[1] is True
        else:
            assert r.move_geometry(plan, DM.skin_dq(old[3], bone, weight, X))[1] is True

    if behind_at_the_mark:
        frame(pt, r, 1)
        move(Xs[0])                                                   # the host copies are behind when the mark is taken
    r.reset_frame()
    r.render_batch(1, seeds_for(pt, 1, 4))
    r.motion_mark()
    move(Xs[1])
    kept = r.reproject_frame_moved()
    carried = r.read_frame().copy()
    r.render_batch(5, seeds_for(pt, 5, 1))
    img = r.read_frame().copy()
    pose.close(); plan.close(); r.close()
    return kept, carried, img


@pytest.mark.parametrize("behind", [False, True], ids=["mark-current", "mark-behind"])
def test_reprojection_workflow_equals_the_twin_s(pt, renderer_mod, m6, behind):
    a = _workflow(pt, renderer_mod, m6, True, behind)
    b = _workflow(pt, renderer_mod, m6, False, behind)
    assert a[0] == b[0] and np.all(np.asarray(a[0]) > 0), (a[0], b[0])      # the kept-pixel count
    same_image(a[1], b[1], "the reprojected image")
    same_image(a[2], b[2], "frames on top")


# ------------------------------------------------------------------------------------------------ refusal, staleness, the slow path

def test_a_zero_length_blend_is_refused_and_the_last_accepted_pose_restored(pt, renderer_mod, soup):
    """Weights (1, -1): on ONE bone the blend has length zero under every pose; on TWO bones it has under the poses that give both the same
    record.  The second table lets one pose object be accepted, refused and restored."""
    old, bone, weight, X1 = soup
    k = int(np.nonzero(bone.reshape(-1, 4)[:, 0] >= 0)[0][0])             # the first moving corner
    bone2, weight2 = bone.copy().reshape(-1, 4), weight.copy().reshape(-1, 4)
    bone2[k], weight2[k] = (0, 1, -1, -1), (1.0, -1.0, np.nan, np.nan)
    bone2, weight2 = bone2.reshape(-1), weight2.reshape(-1)
    bone1, weight1 = bone2.copy(), weight2.copy()
    bone1[4 * k + 1] = 0                                                  # (1, -1) on bone 0 alone
    new1 = posed(old, bone2, weight2, X1)
    same = X1.copy(); same[1] = same[0]
    assert not np.isnan(new1[3]).any() and np.isnan(DM.skin_dq(old[3], bone2, weight2, same).reshape(-1, 40)[k // 3, 4 * (k % 3)])
    assert np.isnan(DM.skin_dq(old[3], bone1, weight1, X1).reshape(-1, 40)[k // 3, 4 * (k % 3)])
    L = renderer_mod.lib()

    def refused(r, pose, X):
        flag = C.c_int(-5)
        cost = np.full(pose.n_roots, -7.0)
        x = np.ascontiguousarray(X, f32)
        rc = L.pt_pose_geometry(r._h, pose._h, x.ctypes.data, x.nbytes, None, 0, cost.ctypes.data, C.byref(flag))
        assert rc == -4 and L.pt_last_error().decode() == NAN_TEXT      # PT_ERR_SCENE: the refusal of every NaN coordinate
        assert flag.value == -5 and (cost == -7.0).all()

    # behind on an accepted pose
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H), asm_node_layout=0)
    frame(pt, r, 1)
    pose = dq_create(r, bone2, weight2, 12)
    one_bone = dq_create(r, bone1, weight1, 12)
    assert r.pose_geometry(pose, X1)[1] is True
    img = frame(pt, r, 2)
    before = records(r)
    refused(r, pose, same)                                                # the same object: its working copies are put back
    same_records(records(r), before, "refused")
    same_image(frame(pt, r, 2), img, "refused")
    refused(r, one_bone, X1)                                              # another object, refused under every pose
    same_records(records(r), before, "refused, one bone")
    same_image(frame(pt, r, 2), img, "refused, one bone")
    r.set_option("asm_node_layout", 1)                                    # a rebuild: the settled copies are the last accepted pose's
    got_img = frame(pt, r, 2)
    want, ref = fresh_records(pt, renderer_mod, new1, MC.SKY, (MC.W, MC.H), asm_node_layout=1)
    same_records(records(r), want, "the settled copies")
    same_image(got_img, ref, "the settled copies")
    one_bone.close(); pose.close(); r.close()
    # no accepted pose yet: the rest pose
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H), asm_node_layout=0)
    img = frame(pt, r, 2)
    before = records(r)
    pose = dq_create(r, bone2, weight2, 12)
    refused(r, pose, same)
    same_records(records(r), before, "refused first")
    same_image(frame(pt, r, 2), img, "refused first")
    assert r.pose_geometry(pose, X1)[1] is True                          # and the pose is still usable
    got_img = frame(pt, r, 2)
    want, ref = fresh_records(pt, renderer_mod, new1, MC.SKY, (MC.W, MC.H), asm_node_layout=0)
    same_records(records(r), want, "a good pose after the refusal")
    same_image(got_img, ref, "a good pose after the refusal")
    pose.close(); r.close()


def test_a_dq_pose_is_stale_after_an_upload_of_binding_3(pt, renderer_mod, soup):
    old, bone, weight, X = soup
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
    frame(pt, r, 1)
    pose = dq_create(r, bone, weight, 12)
    assert r.pose_geometry(pose, X)[1] is True
    r.set_buffer(3, old[3])
    with pytest.raises(renderer_mod.PtError) as e:
        r.pose_geometry(pose, X)
    assert e.value.code == -4 and "the scene was uploaded since pt_pose_create" in str(e.value)
    again = dq_create(r, bone, weight, 12)                                # a new pose over the uploaded scene works
    assert r.pose_geometry(again, X)[1] is True
    frame(pt, r, 2)
    same_records(records(r), fresh_records(pt, renderer_mod, posed(old, bone, weight, X), MC.SKY, (MC.W, MC.H))[0], "a new pose after the upload")
    r.close()


def test_slow_path_multi_stream_context(pt, renderer_mod, m6):
    rest, old, tex, bone, weight, Xs = m6
    new = posed(old, bone, weight, Xs[1])
    r = renderer_mod.Renderer(rest.W, rest.H, devices=[0, 0])
    r.load_workload(rest)
    frame(pt, r, 1)
    pose = dq_create(r, bone, weight, 5)
    plan = renderer_mod.RefitPlan(old)
    cost, in_place = r.pose_geometry(pose, Xs[1])
    assert in_place is False
    assert np.array_equal(cost.view(np.uint64), plan.run(new[3])[1].view(np.uint64))
    same_floats(pose.triangles(Xs[1]), new[3], "multi")
    img = frame(pt, r, 2)
    pose.close(); plan.close(); r.close()
    single = context(renderer_mod, old, tex, (rest.W, rest.H))            # the single-stream frames of the same pose
    frame(pt, single, 1)
    one = dq_create(single, bone, weight, 5)
    assert single.pose_geometry(one, Xs[1])[1] is True
    ref = frame(pt, single, 2)
    one.close(); single.close()
    same_image(img, ref, "multi")


def test_the_debug_timers_refuse_the_poses_of_the_other_rules(pt, renderer_mod, soup):
    old, bone, weight, X = soup
    L = renderer_mod.lib()
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
    dq = dq_create(r, bone, weight, 12)
    linear = r.skin_create(bone, weight, 12)
    assert linear.blend == "linear"
    part = r.pose_create(PM.parts_mod4(old[3].size // 40), 12)
    x = np.ascontiguousarray(X, f32).reshape(-1)
    best = C.c_float(-2.0)
    for which in (0, 1):
        assert L.pt_debug_pose_time(dq._h, x.ctypes.data, x.nbytes, which, 1, C.byref(best)) == -1      # PT_ERR_ARG
        assert L.pt_last_error().decode().startswith("pt_debug_pose_time: ") and best.value == -2.0
        assert L.pt_debug_skin_time(dq._h, x.ctypes.data, x.nbytes, which, 1, C.byref(best)) == -1
        assert L.pt_last_error().decode().startswith("pt_debug_skin_time: ") and best.value == -2.0
    for other in (part, linear):
        assert L.pt_debug_skin_dq_time(other._h, x.ctypes.data, x.nbytes, 1, C.byref(best)) == -1
        assert L.pt_last_error().decode() == "pt_debug_skin_dq_time: bad argument" and best.value == -2.0
    assert L.pt_debug_skin_dq_time(dq._h, x.ctypes.data, x.nbytes, 0, C.byref(best)) == -1 and best.value == -2.0      # reps < 1
    assert L.pt_debug_skin_dq_time(dq._h, x.ctypes.data, x.nbytes, 1, C.byref(best)) == 0, L.pt_last_error()
    assert best.value >= 0.0
    same_floats(scratch(r, dq), DM.skin_dq(old[3], bone, weight, X), "timed launches")
    same_floats(linear.triangles(X), SM.skin(old[3], bone, weight, X), "the linear skin beside it is the linear skin")
    part.close(); linear.close(); dq.close(); r.close()
