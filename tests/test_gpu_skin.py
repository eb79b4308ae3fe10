"""GPU: include/pt_skin.h — pt_pose_triangles of a skinned pose against the numpy model of the rule (tests/_skin_model.py), both device statements
through pt_debug_skin_time, and pt_pose_geometry of a skinned pose against a twin context on which move_geometry(plan, model_skinned) ran: every
device record array byte for byte, the frames, root_cost, the reprojection workflow, a rebuild from the settled copies, the refusal and what it
restores, staleness, the multi-stream slow path.  48 x 27 or 96 x 54, a few frames.

A NaN the rule generates (inf * 0, inf - inf) equals any NaN: its sign and payload are the hardware's, and the model runs on another.  Everything
else is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _move_cases as MC
import _pose_model as PM
import _skin_model as SM
from test_gpu_move import context, frame, records, same_image, same_records
from test_gpu_parity import seeds_for
from test_gpu_pose import fresh_records, one_soup, same_floats
from test_scene_layout import leaf_roots

pytestmark = pytest.mark.gpu

f32 = np.float32
_CACHE = {}


def skin_create(r, bone, weight, n_parts):
    assert hasattr(r._L, "pt_skin_create") and hasattr(r, "skin_create")      # never skipped: a library without the symbol fails here
    return r.skin_create(bone, weight, n_parts)


def scene_of(pt, n):
    """a complete scene of ONE object of n triangles (one triangle: a leaf root made by hand, the builder makes none)"""
    if n > 1:
        return one_soup(pt, n)
    if "one" not in _CACHE:
        b = dict(leaf_roots(1)[0])
        b[3] = b[3].copy(); b[3][[14, 18, 22]] = 1.0
        _CACHE["one"] = MC.complete(pt, b)
    return _CACHE["one"]


def skinned(old, bone, weight, X):
    """the scene after the skin, by the models: binding 3 by the rule, binding 10 by the refit model"""
    key = ("skinned", id(old[3]), bone.tobytes(), weight.tobytes(), np.ascontiguousarray(X, f32).tobytes())
    if key not in _CACHE:
        new = dict(old)
        new[3], new[10] = MC.move_of(old, SM.skin(old[3], bone, weight, X))
        _CACHE[key] = (old[3], new)
    return _CACHE[key][1]


def scratch(r, pose):
    out = np.empty(pose.n_tris * 40, f32)
    assert r._L.pt_debug_pose_scratch(pose._h, out.ctypes.data, out.nbytes) == 0, r._L.pt_last_error()
    return out


def both_statements(r, pose, X, want, tag):
    """pt_debug_skin_time fills the scratch copy with the rest pose and then runs the statement asked for: what lies there is that kernel's"""
    x = np.ascontiguousarray(X, f32).reshape(-1)
    for which in (0, 1):
        best = C.c_float(-1.0)
        assert r._L.pt_debug_skin_time(pose._h, x.ctypes.data, x.nbytes, which, 1, C.byref(best)) == 0, r._L.pt_last_error()
        assert best.value >= 0.0
        same_floats(scratch(r, pose), want, (tag, "statement", which))


# ------------------------------------------------------------------------------------------------ the rule alone

@pytest.mark.parametrize("n", [1, 2, 42, 43, 44, 85, 86, 255, 256, 257, 1000])
def test_skin_triangles_equals_the_model(pt, renderer_mod, n):
    """one lane per float4, 256 lanes per block: a block ends inside triangle 42 (the 43rd), and with one lane per corner inside triangle 85.  Every
    third triangle holds +-0, denormals, +-inf and 3e38; 0-4 slots per corner, so static corners lie inside moving triangles and the weights of
    empty slots are NaN; the trees are the ordinary soup's."""
    b = dict(scene_of(pt, n))
    t = b[3].reshape(-1, 40).copy()
    t[::3, :24] = PM.special_triangles(len(t[::3]), seed=n).reshape(-1, 40)[:, :24]
    b[3] = t.reshape(-1)
    bone, weight = SM.random_skin(n, 3, seed=n)
    r = context(renderer_mod, b, MC.SKY, (MC.W, MC.H))
    pose = skin_create(r, bone, weight, 3)
    static = np.repeat(bone.reshape(-1, 4)[:, 0] < 0, 4).reshape(-1, 3, 4)      # per triangle, per corner: its float4 (vertex, and normal 12 on)
    keep = np.zeros((n, 40), bool); keep[:, :12] = static.reshape(n, 12); keep[:, 12:24] = static.reshape(n, 12); keep[:, 24:] = True
    for seed in (5, 6):
        X = PM.matrices(3, seed)
        got = pose.triangles(X)
        want = SM.skin(b[3], bone, weight, X)
        same_floats(got, want, (n, seed))
        assert np.array_equal(got.view(np.uint32)[keep.reshape(-1)], b[3].view(np.uint32)[keep.reshape(-1)])      # static corners: the rest pose's bits
    both_statements(r, pose, X, want, n)
    X = PM.matrices(3, 7); X[0, :21] = PM.SPECIAL[np.arange(21) % PM.SPECIAL.size]; X[2, 3] = np.inf
    want = SM.skin(b[3], bone, weight, X)
    same_floats(pose.triangles(X), want, (n, "special matrices"))
    both_statements(r, pose, X, want, (n, "special matrices"))
    none = skin_create(r, *SM.random_skin(n, 0), 0)
    assert np.array_equal(none.triangles(np.zeros(0, f32)).view(np.uint32), b[3].view(np.uint32))      # n_parts = 0: the rest pose
    none.close(); pose.close(); r.close()


@pytest.mark.parametrize("n_parts", [1, 65536])
def test_skin_triangles_with_one_bone_and_with_65536(pt, renderer_mod, n_parts):
    n = 257
    b = one_soup(pt, n)
    bone, weight = SM.random_skin(n, n_parts, seed=n_parts % 97, top_bone=True)
    assert bone.max() == n_parts - 1
    rng = np.random.RandomState(n_parts % 89)
    X = np.zeros((n_parts, 24), f32)
    X[:] = PM.matrices(1, 3)[0]
    X[:, :21] += rng.uniform(-0.1, 0.1, (n_parts, 21)).astype(f32)
    r = context(renderer_mod, b, MC.SKY, (MC.W, MC.H))
    pose = skin_create(r, bone, weight, n_parts)
    want = SM.skin(b[3], bone, weight, X)
    same_floats(pose.triangles(X), want, n_parts)
    both_statements(r, pose, X, want, n_parts)
    pose.close(); r.close()


def test_the_weight_1_skin_equals_pose_triangles(pt, renderer_mod):
    n = 257
    b = dict(one_soup(pt, n))
    t = b[3].reshape(-1, 40).copy()
    t[::3, :24] = PM.special_triangles(len(t[::3]), seed=9).reshape(-1, 40)[:, :24]
    b[3] = t.reshape(-1)
    parts = PM.parts_mod4(n)
    r = context(renderer_mod, b, MC.SKY, (MC.W, MC.H))
    pose = r.pose_create(parts, 3)
    skin = skin_create(r, *SM.skin_of_parts(parts), 3)
    for seed in (5, 6):
        X = PM.matrices(3, seed)
        want = pose.triangles(X)
        same_floats(skin.triangles(X), want, seed)
        same_floats(want, PM.pose(b[3], parts, X), (seed, "the pose itself"))
    skin.close(); pose.close(); r.close()


# ------------------------------------------------------------------------------------------------ records and frames against the twin

def skin_equals_twin(pt, renderer_mod, old, tex, size, bone, weight, n_parts, X, tag, **opts):
    P = SM.skin(old[3], bone, weight, X)
    out = []
    for twin in (False, True):
        r = context(renderer_mod, old, tex, size, **opts)
        frame(pt, r, 1)
        if twin:
            plan = renderer_mod.RefitPlan(old)
            cost, in_place = r.move_geometry(plan, P)
        else:
            pose = skin_create(r, bone, weight, n_parts)
            cost, in_place = r.pose_geometry(pose, X)
        assert in_place is True, (tag, twin)
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


@pytest.fixture(scope="module")
def soup(pt):
    old = MC.scenes(pt)["soup129"]
    bone, weight = SM.random_skin(old[3].size // 40, 3, seed=41)
    return old, bone, weight, PM.matrices(3)


@pytest.fixture(scope="module")
def m3(pt):
    """(M3's rest workload, its buffers and textures, the two tables, the records of two steps)"""
    rest, bone, weight, X2 = pt.scenes.m3_bending(2)
    old, tex = MC.workload_inputs(rest)
    return rest, old, tex, bone, weight, [X2, pt.scenes.m3_bending(4)[3]]


@pytest.mark.parametrize("opts", [{}, dict(bfs_nodes=3)], ids=["default", "bfs3"])
def test_records_equal_the_twin_s_on_a_soup(pt, renderer_mod, soup, opts):
    old, bone, weight, X = soup
    got = skin_equals_twin(pt, renderer_mod, old, MC.SKY, (MC.W, MC.H), bone, weight, 3, X, ("soup129", opts), **opts)
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H), **opts)
    frame(pt, r, 1)
    was = records(r)
    assert not (np.array_equal(got["tris"], was["tris"]) or np.array_equal(got["shade"], was["shade"]))      # the skin did move something
    r.close()


@pytest.mark.parametrize("opts", [{}, dict(bfs_nodes=3)], ids=["default", "bfs3"])
def test_records_equal_the_twin_s_on_m3(pt, renderer_mod, m3, opts):
    rest, old, tex, bone, weight, Xs = m3
    skin_equals_twin(pt, renderer_mod, old, tex, (rest.W, rest.H), bone, weight, 5, Xs[1], ("M3", opts), **opts)


def test_two_frames_root_cost_and_in_place_equal_the_twin_s(pt, renderer_mod, m3):
    rest, old, tex, bone, weight, Xs = m3
    P = SM.skin(old[3], bone, weight, Xs[1])
    seeds = seeds_for(pt, 1, 2)
    L = renderer_mod.lib()
    out = []
    for twin in (False, True):
        r = context(renderer_mod, old, tex, (rest.W, rest.H))
        frame(pt, r, 1)
        if twin:
            plan = renderer_mod.RefitPlan(old)
            cost, in_place = r.move_geometry(plan, P)
            assert in_place is True
        else:
            pose = skin_create(r, bone, weight, 5)
            flag = C.c_int(-5)
            cost = np.full(pose.n_roots, -7.0)
            x = np.ascontiguousarray(Xs[1], f32)
            assert L.pt_pose_geometry(r._h, pose._h, x.ctypes.data, x.nbytes, None, 0, cost.ctypes.data, C.byref(flag)) == 0, L.pt_last_error()
            assert flag.value == 1                                      # in_place == 1
        r.set_option("count_stats", 1)
        r.reset_frame(); r.reset_counters()
        r.render_batch(1, seeds)
        counted, cnt = r.read_frame(), r.counters()
        r.set_option("count_stats", 0)
        r.reset_frame()
        r.render_batch(1, seeds)
        out.append((counted, cnt, r.read_frame(), cost))
        (plan if twin else pose).close(); r.close()
    same_image(out[0][0], out[1][0], "counting kernels")
    same_image(out[0][2], out[1][2], "shipped kernels")
    same_image(out[0][0], out[0][2], "shipped kernels against the counting variants")
    assert out[0][1] == out[1][1] and out[0][0][..., :3].max() > 0
    assert out[0][3].size == int(old[13][0]) > 0 and np.array_equal(out[0][3].view(np.uint64), out[1][3].view(np.uint64))      # root_cost


# ------------------------------------------------------------------------------------------------ the moving-geometry workflow

def _workflow(pt, renderer_mod, m3, by_skin, behind_at_the_mark):
    """mark -> skin -> reproject_frame_moved -> one frame"""
    rest, old, tex, bone, weight, Xs = m3
    r = context(renderer_mod, old, tex, (rest.W, rest.H))
    plan = renderer_mod.RefitPlan(old)
    pose = skin_create(r, bone, weight, 5)

    def move(X):
        if by_skin:
            assert r.pose_geometry(pose, X)[1] is True
        else:
            assert r.move_geometry(plan, SM.skin(old[3], bone, weight, X))[1] is True

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
def test_reprojection_workflow_equals_the_twin_s(pt, renderer_mod, m3, behind):
    a = _workflow(pt, renderer_mod, m3, True, behind)
    b = _workflow(pt, renderer_mod, m3, False, behind)
    assert a[0] == b[0] and np.all(np.asarray(a[0]) > 0), (a[0], b[0])      # the kept-pixel count
    same_image(a[1], b[1], "the reprojected image")
    same_image(a[2], b[2], "one frame on top")


# ------------------------------------------------------------------------------------------------ the host copies

def test_a_rebuild_after_a_skin_reads_the_settled_copies(pt, renderer_mod, soup):
    old, bone, weight, X = soup
    new = skinned(old, bone, weight, X)
    want, ref = fresh_records(pt, renderer_mod, new, MC.SKY, (MC.W, MC.H), asm_node_layout=1)
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
    frame(pt, r, 1)
    pose = skin_create(r, bone, weight, 3)
    assert r.pose_geometry(pose, X)[1] is True
    r.set_option("asm_node_layout", 1)                                # dirties the scene: the next render lays it out from the settled copies
    img = frame(pt, r, 2)
    same_records(records(r), want, "option")
    same_image(img, ref, "option")
    pose.close(); r.close()


# ------------------------------------------------------------------------------------------------ refusal, staleness, the slow path

def test_a_refusal_leaves_records_and_image_and_restores_the_last_accepted_skin(pt, renderer_mod, soup):
    old, bone, weight, X1 = soup
    new1 = skinned(old, bone, weight, X1)
    L = renderer_mod.lib()
    inf = X1.copy(); inf[0, 0] = np.inf; inf[0, 1] = -np.inf          # w * inf stays infinite; inf * x - inf * y: a NaN wherever x and y have the same sign
    with np.errstate(all="ignore"):
        bad = SM.skin(old[3], bone, weight, inf).reshape(-1, 40)
    assert np.isnan(bad[:, :11]).any() and not np.isnan(SM.skin(old[3], bone, weight, X1)).any()

    def refused(r, pose):
        flag = C.c_int(-5)
        cost = np.full(pose.n_roots, -7.0)
        x = np.ascontiguousarray(inf, f32)
        rc = L.pt_pose_geometry(r._h, pose._h, x.ctypes.data, x.nbytes, None, 0, cost.ctypes.data, C.byref(flag))
        assert rc == -4 and L.pt_last_error().decode() == "pt_pose_geometry: NaN coordinate in a referenced triangle"      # PT_ERR_SCENE
        assert flag.value == -5 and (cost == -7.0).all()

    # behind on an accepted skin
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H), asm_node_layout=0)
    frame(pt, r, 1)
    pose = skin_create(r, bone, weight, 3)
    assert r.pose_geometry(pose, X1)[1] is True
    img = frame(pt, r, 2)
    before = records(r)
    refused(r, pose)
    same_records(records(r), before, "refused")
    same_image(frame(pt, r, 2), img, "refused")
    r.set_option("asm_node_layout", 1)                                # a rebuild: the settled copies are the last accepted skin's
    got_img = frame(pt, r, 2)
    want, ref = fresh_records(pt, renderer_mod, new1, MC.SKY, (MC.W, MC.H), asm_node_layout=1)
    same_records(records(r), want, "the settled copies")
    same_image(got_img, ref, "the settled copies")
    pose.close(); r.close()
    # no accepted pose yet: the rest pose
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H), asm_node_layout=0)
    img = frame(pt, r, 2)
    before = records(r)
    pose = skin_create(r, bone, weight, 3)
    refused(r, pose)
    same_records(records(r), before, "refused first")
    same_image(frame(pt, r, 2), img, "refused first")
    r.set_option("asm_node_layout", 1)
    got_img = frame(pt, r, 2)
    want, ref = fresh_records(pt, renderer_mod, old, MC.SKY, (MC.W, MC.H), asm_node_layout=1)
    same_records(records(r), want, "the rest pose")
    same_image(got_img, ref, "the rest pose")
    assert r.pose_geometry(pose, X1)[1] is True                      # and the skin is still usable
    got_img = frame(pt, r, 2)
    want, ref = fresh_records(pt, renderer_mod, new1, MC.SKY, (MC.W, MC.H), asm_node_layout=1)
    same_records(records(r), want, "a good skin after the refusal")
    same_image(got_img, ref, "a good skin after the refusal")
    pose.close(); r.close()


def test_a_skin_is_stale_after_an_upload_of_binding_3(pt, renderer_mod, soup):
    old, bone, weight, X = soup
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
    frame(pt, r, 1)
    pose = skin_create(r, bone, weight, 3)
    assert r.pose_geometry(pose, X)[1] is True
    r.set_buffer(3, old[3])
    with pytest.raises(renderer_mod.PtError) as e:
        r.pose_geometry(pose, X)
    assert e.value.code == -4 and "the scene was uploaded since pt_pose_create" in str(e.value)
    again = skin_create(r, bone, weight, 3)                           # a new skin over the uploaded scene works
    assert r.pose_geometry(again, X)[1] is True
    frame(pt, r, 2)
    same_records(records(r), fresh_records(pt, renderer_mod, skinned(old, bone, weight, X), MC.SKY, (MC.W, MC.H))[0], "a new skin after the upload")
    r.close()


def test_slow_path_multi_stream_context(pt, renderer_mod, m3):
    rest, old, tex, bone, weight, Xs = m3
    new = skinned(old, bone, weight, Xs[1])
    r = renderer_mod.Renderer(rest.W, rest.H, devices=[0, 0])
    r.load_workload(rest)
    frame(pt, r, 1)
    pose = skin_create(r, bone, weight, 5)
    plan = renderer_mod.RefitPlan(old)
    cost, in_place = r.pose_geometry(pose, Xs[1])
    assert in_place is False
    assert np.array_equal(cost.view(np.uint64), plan.run(new[3])[1].view(np.uint64))
    same_floats(pose.triangles(Xs[1]), new[3], "multi")
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


def test_debug_pose_time_refuses_a_skinned_pose(pt, renderer_mod, soup):
    old, bone, weight, X = soup
    L = renderer_mod.lib()
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
    skin = skin_create(r, bone, weight, 3)
    pose = r.pose_create(PM.parts_mod4(old[3].size // 40), 3)
    x = np.ascontiguousarray(X, f32).reshape(-1)
    best = C.c_float(-2.0)
    for which in (0, 1):
        assert L.pt_debug_pose_time(skin._h, x.ctypes.data, x.nbytes, which, 1, C.byref(best)) == -1      # PT_ERR_ARG
        assert L.pt_last_error().decode().startswith("pt_debug_pose_time: ") and best.value == -2.0
        assert L.pt_debug_skin_time(pose._h, x.ctypes.data, x.nbytes, which, 1, C.byref(best)) == -1      # and the other way round
    for which in (0, 1):
        assert L.pt_debug_pose_time(pose._h, x.ctypes.data, x.nbytes, which, 1, C.byref(best)) == 0, L.pt_last_error()
        assert best.value >= 0.0
    skin.close(); pose.close(); r.close()
