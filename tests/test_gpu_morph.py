"""GPU: include/pt_morph.h — the kernel alone (pt_debug_morph_rest) against the numpy model of the rule (tests/_morph_model.py),
pt_pose_triangles of a morphed pose against the model chained with the pose and the skin models, and pt_pose_geometry of a morphed pose against a
twin context on which move_geometry(plan, model_triangles) ran: every device record array byte for byte, the frames, root_cost, the reprojection
workflow, the refusal and what it restores (records AND weights), staleness, the attach-time refusals that need a device-made pose, the
multi-stream slow path.  48 x 27 or 96 x 54, a few frames.

A NaN the rule generates equals any NaN: its sign and payload are the hardware's, and the model runs on another.  Everything else is compared bit
for bit."""
import ctypes as C

import numpy as np
import pytest

import _morph_model as MM
import _move_cases as MC
import _pose_model as PM
import _skin_model as SM
from test_gpu_move import context, frame, records, same_image, same_records
from test_gpu_parity import seeds_for
from test_gpu_pose import fresh_records, one_soup, same_floats
from test_gpu_skin import scene_of

pytestmark = pytest.mark.gpu

f32 = np.float32


def attach(pose, targets):
    assert hasattr(pose._L, "pt_morph_attach") and hasattr(pose, "morph_attach")      # never skipped: a library without the symbol fails here
    pose.morph_attach(targets)
    return pose


def morph_rest(pose):
    out = np.empty(pose.n_tris * 40, f32)
    assert pose._L.pt_debug_morph_rest(pose._h, out.ctypes.data, out.nbytes) == 0, pose._L.pt_last_error()
    return out


def same_bits(a, b, tag):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), tag


def with_specials(b, seed):
    """every third triangle holds +-0, denormals, +-inf and 3e38 in its vertex and normal floats; the trees are the ordinary scene's"""
    b = dict(b)
    t = b[3].reshape(-1, 40).copy()
    t[::3, :24] = PM.special_triangles(len(t[::3]), seed=seed).reshape(-1, 40)[:, :24]
    b[3] = t.reshape(-1)
    return b


def make_pose(r, kind, n, seed=1):
    """(pose, the corners its rule moves, a function rest -> posed by the model, records).  all: one part; mod4: a quarter of the triangles static;
    skin: 0-4 slots per corner, so static corners lie inside moving triangles"""
    if kind == "skin":
        bone, weight = SM.random_skin(n, 3, seed=seed)
        X = PM.matrices(3, 5)
        return r.skin_create(bone, weight, 3), MM.moved_corners(n, bone=bone), (lambda rest, X=X: SM.skin(rest, bone, weight, X)), X
    parts = np.zeros(n, np.int32) if kind == "all" else PM.parts_mod4(n)
    n_parts = 1 if kind == "all" else 3
    X = PM.matrices(n_parts, 5)
    return r.pose_create(parts, n_parts), MM.moved_corners(n, tri_part=parts), (lambda rest, X=X: PM.pose(rest, parts, X)), X


# ------------------------------------------------------------------------------------------------ the kernel alone

KERNEL_CASES = [(1, "all", 1, 1), (1, "all", 2, 3), (86, "all", 255, 3), (86, "all", 256, 1), (86, "all", 257, 3), (257, "mod4", 256, 1024), (257, "mod4", 257, 3),
                (1000, "skin", 1000, 3), (1000, "skin", 300, 1024)]


@pytest.mark.parametrize("n, kind, n_affected, n_targets", KERNEL_CASES)
def test_the_kernel_alone_equals_the_model(pt, renderer_mod, n, kind, n_affected, n_targets):
    """one lane per affected corner, 256 lanes per block: 255, 256 and 257 affected corners end before, at and after a block's last lane.  Rows
    of uneven length, one corner named by every target, the entries shuffled within the targets; +0, -0, denormals, negatives and 2.0 among the
    weights.  What is unaffected or static keeps the rest pose's bits."""
    b = with_specials(scene_of(pt, n), seed=n + n_targets)
    r = context(renderer_mod, b, MC.SKY, (MC.W, MC.H))
    pose, allowed, _, _ = make_pose(r, kind, n, seed=n)
    targets, affected = MM.random_targets(allowed, n_affected, n_targets, seed=n_affected + n_targets)
    assert affected.size == n_affected and len(targets) == n_targets
    lengths = np.bincount(np.concatenate([c for c, _ in targets]), minlength=3 * n)[affected]
    assert lengths.max() == n_targets and (n_affected < 50 or n_targets == 1 or lengths.min() < lengths.max())
    attach(pose, targets)
    same_bits(morph_rest(pose), b[3], (n, "after the attach every weight is 0"))
    keep = np.ones((n, 40), bool)
    k, c = affected // 3, affected % 3
    for j in range(3):
        keep[k, 4 * c + j] = False; keep[k, 12 + 4 * c + j] = False
    rest_bits = b[3].view(np.uint32)
    for seed in (4, 5):
        w = MM.special_weights(n_targets, seed)
        pose.morph_weights(w)
        got = morph_rest(pose)
        same_floats(got, MM.morph(b[3], targets, w), (n, kind, n_affected, n_targets, seed))
        assert np.array_equal(got.view(np.uint32)[keep.reshape(-1)], rest_bits[keep.reshape(-1)])
    best = C.c_float(-1.0)
    other = np.full(n_targets, 0.5, f32)
    assert pose._L.pt_debug_morph_time(pose._h, other.ctypes.data, other.nbytes, 2, C.byref(best)) == 0, pose._L.pt_last_error()
    assert best.value >= 0.0
    same_floats(morph_rest(pose), MM.morph(b[3], targets, w), (n, "the weights last set, after the timer ran under others"))
    pose.morph_weights(np.zeros(n_targets, f32))
    same_bits(morph_rest(pose), b[3], (n, "back to zero: every affected corner is rewritten"))
    pose.close(); r.close()


# ------------------------------------------------------------------------------------------------ the chain

@pytest.mark.parametrize("kind", ["mod4", "skin"])
def test_pose_triangles_equals_the_chained_models(pt, renderer_mod, kind):
    n = 257
    b = with_specials(one_soup(pt, n), seed=11)
    r = context(renderer_mod, b, MC.SKY, (MC.W, MC.H))
    pose, allowed, model, X = make_pose(r, kind, n, seed=3)
    plain = make_pose(r, kind, n, seed=3)[0]                             # the same pose without a morph, on the same context
    targets, affected = MM.random_targets(allowed, 300, 5, seed=8)
    attach(pose, targets)
    unmorphed = plain.triangles(X)
    same_floats(unmorphed, model(b[3]), (kind, "the pose alone"))
    same_bits(pose.triangles(X), unmorphed, (kind, "consequence 1: after the attach"))
    w1, w2 = MM.special_weights(5, 1), np.array([2.0, -0.75, 0.0, 1.0, 1e-39], f32)
    seen = {}
    for tag, w in (("w1", w1), ("+-0", np.array([0.0, -0.0, -0.0, 0.0, -0.0], f32)), ("w1", w1), ("w2", w2), ("w1", w1)):
        pose.morph_weights(w)
        got = pose.triangles(X)
        if tag == "+-0":
            same_bits(got, unmorphed, (kind, "consequence 1"))           # -0.0 and infinities of the rest pose included
            continue
        same_floats(got, model(MM.morph(b[3], targets, w)), (kind, tag))
        if tag in seen:
            same_bits(got, seen[tag], (kind, tag, "set, set back, set again: nothing stale in the morphed copy"))
        seen[tag] = got
    assert not np.array_equal(seen["w1"].view(np.uint32), seen["w2"].view(np.uint32))
    static = np.ones(3 * n, bool); static[allowed] = False
    assert static.any()
    for q in np.nonzero(static)[0][:50]:                                  # static corners: the rest pose's bits
        k, c = divmod(int(q), 3)
        same_bits(seen["w1"].reshape(-1, 40)[k, 4 * c:4 * c + 4], b[3].reshape(-1, 40)[k, 4 * c:4 * c + 4], q)
        same_bits(seen["w1"].reshape(-1, 40)[k, 12 + 4 * c:16 + 4 * c], b[3].reshape(-1, 40)[k, 12 + 4 * c:16 + 4 * c], q)
    same_bits(plain.triangles(X), unmorphed, "the unmorphed pose beside it is untouched")
    plain.close(); pose.close(); r.close()


@pytest.fixture(scope="module")
def m4(pt):
    """(M4's rest workload, its buffers and textures, the skin tables, the targets, per step (records, weights))"""
    rest, bone, weight, targets, X, w = pt.scenes.m4_bulging(1)
    old, tex = MC.workload_inputs(rest)
    steps = [(X, w)] + [pt.scenes.m4_bulging(s)[4:] for s in (3, 7)]
    return rest, old, tex, bone, weight, targets, steps


def test_shared_corners_of_m4_get_the_same_bits(pt, renderer_mod, m4):
    rest, old, tex, bone, weight, targets, steps = m4
    r = context(renderer_mod, old, tex, (rest.W, rest.H))
    pose = attach(r.skin_create(bone, weight, 5), targets)
    words = [bone.reshape(-1, 4)[q].tobytes() + weight.reshape(-1, 4)[q].tobytes() for q in range(bone.size // 4)]
    for X, w in steps:
        pose.morph_weights(w)
        got = pose.triangles(X)
        same_floats(got, MM.morph_skin(old[3], targets, w, bone, weight, X), "M4")
        cracks, shared = MM.shared_corners_crack(got, old[3], targets, words)
        assert cracks == 0 and shared > 100, (cracks, shared)
    pose.close(); r.close()


# ------------------------------------------------------------------------------------------------ records and frames against the twin

def morph_equals_twin(pt, renderer_mod, old, tex, size, create, targets, w, X, P, tag, **opts):
    out = []
    for twin in (False, True):
        r = context(renderer_mod, old, tex, size, **opts)
        frame(pt, r, 1)
        if twin:
            plan = renderer_mod.RefitPlan(old)
            cost, in_place = r.move_geometry(plan, P)
        else:
            pose = attach(create(r), targets)
            pose.morph_weights(w)
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
    same_image(img, img2, tag)                                            # two frames
    return got


@pytest.fixture(scope="module")
def soup(pt):
    """(soup129, a skin over it, targets on the corners it moves — the last one far too large, with weight 0 wherever the pose is to be
    accepted —, records, two weight vectors)"""
    old = MC.scenes(pt)["soup129"]
    n = old[3].size // 40
    bone, weight = SM.random_skin(n, 3, seed=41)
    targets, _ = MM.random_targets(MM.moved_corners(n, bone=bone), 200, 4, seed=6, scale=0.2)
    c, d = targets[0]
    targets.append((c.copy(), (d * f32(1e30)).astype(f32)))
    return old, bone, weight, targets, PM.matrices(3), [np.array([0.8, -0.5, 1e-39, 1.5, 0.0], f32), np.array([0.0, 1.0, 0.25, -0.0, 0.0], f32)]


@pytest.mark.parametrize("opts", [{}, dict(bfs_nodes=3)], ids=["default", "bfs3"])
def test_records_equal_the_twin_s_on_a_soup(pt, renderer_mod, soup, opts):
    old, bone, weight, targets, X, ws = soup
    P = MM.morph_skin(old[3], targets, ws[0], bone, weight, X)
    assert not np.isnan(P).any() and not np.array_equal(P, SM.skin(old[3], bone, weight, X))      # the morph did move something
    morph_equals_twin(pt, renderer_mod, old, MC.SKY, (MC.W, MC.H), lambda r: r.skin_create(bone, weight, 3), targets, ws[0], X, P, ("soup129", opts), **opts)


@pytest.mark.parametrize("opts", [{}, dict(bfs_nodes=3)], ids=["default", "bfs3"])
def test_records_equal_the_twin_s_on_a_soup_under_a_part_pose(pt, renderer_mod, soup, opts):
    old, _, _, _, X, ws = soup
    n = old[3].size // 40
    parts = PM.parts_mod4(n)
    targets, _ = MM.random_targets(MM.moved_corners(n, tri_part=parts), 150, 3, seed=9, scale=0.2)
    P = MM.morph_pose(old[3], targets, ws[0][:3], parts, X)
    morph_equals_twin(pt, renderer_mod, old, MC.SKY, (MC.W, MC.H), lambda r: r.pose_create(parts, 3), targets, ws[0][:3], X, P, ("soup129 parts", opts), **opts)


@pytest.mark.parametrize("opts", [{}, dict(bfs_nodes=3)], ids=["default", "bfs3"])
def test_records_equal_the_twin_s_on_m4(pt, renderer_mod, m4, opts):
    rest, old, tex, bone, weight, targets, steps = m4
    X, w = steps[1]
    P = MM.morph_skin(old[3], targets, w, bone, weight, X)
    assert not np.array_equal(P, SM.skin(old[3], bone, weight, X))
    morph_equals_twin(pt, renderer_mod, old, tex, (rest.W, rest.H), lambda r: r.skin_create(bone, weight, 5), targets, w, X, P, ("M4", opts), **opts)


# ------------------------------------------------------------------------------------------------ the moving-geometry workflow

def _workflow(pt, renderer_mod, m4, by_morph, behind_at_the_mark):
    """mark -> morphed pose -> reproject_frame_moved -> one frame"""
    rest, old, tex, bone, weight, targets, steps = m4
    r = context(renderer_mod, old, tex, (rest.W, rest.H))
    plan = renderer_mod.RefitPlan(old)
    pose = attach(r.skin_create(bone, weight, 5), targets)

    def move(X, w):
        if by_morph:
            pose.morph_weights(w)
            assert r.pose_geometry(pose, X)[1] is True
        else:
            assert r.move_geometry(plan, MM.morph_skin(old[3], targets, w, bone, weight, X))[1] is True

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
def test_reprojection_workflow_equals_the_twin_s(pt, renderer_mod, m4, behind):
    a = _workflow(pt, renderer_mod, m4, True, behind)
    b = _workflow(pt, renderer_mod, m4, False, behind)
    assert a[0] == b[0] and np.all(np.asarray(a[0]) > 0), (a[0], b[0])      # the kept-pixel count
    same_image(a[1], b[1], "the reprojected image")
    same_image(a[2], b[2], "one frame on top")


# ------------------------------------------------------------------------------------------------ refusal and restore

def test_a_refusal_leaves_records_and_image_and_restores_the_last_accepted_records_and_weights(pt, renderer_mod, soup):
    old, bone, weight, targets, X, ws = soup
    L = renderer_mod.lib()
    w1 = ws[0]
    huge = np.array([0.0, 0.0, 0.0, 0.0, 3e38], f32)                     # 3e38 * (0.2e30) overflows: +-inf in the morphed rest pose, NaN after the skin
    P1 = MM.morph_skin(old[3], targets, w1, bone, weight, X)
    with np.errstate(all="ignore"):
        bad = MM.morph_skin(old[3], targets, huge, bone, weight, PM.matrices(3, 6)).reshape(-1, 40)
    assert np.isnan(bad[:, :11]).any() and np.isinf(MM.morph(old[3], targets, huge)).any() and not np.isnan(P1).any()
    new1 = dict(old)
    new1[3], new1[10] = MC.move_of(old, P1)
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H), asm_node_layout=0)
    frame(pt, r, 1)
    pose = attach(r.skin_create(bone, weight, 3), targets)
    pose.morph_weights(w1)
    assert r.pose_geometry(pose, X)[1] is True                           # an accepted pose with non-zero weights
    img = frame(pt, r, 2)
    before = records(r)
    pose.morph_weights(huge)                                              # accepted: nothing is refused before the rule runs
    flag = C.c_int(-5)
    cost = np.full(pose.n_roots, -7.0)
    x = np.ascontiguousarray(PM.matrices(3, 6), f32)                      # other records too: the restore needs the accepted ones AND the accepted weights
    rc = L.pt_pose_geometry(r._h, pose._h, x.ctypes.data, x.nbytes, None, 0, cost.ctypes.data, C.byref(flag))
    assert rc == -4 and L.pt_last_error().decode() == "pt_pose_geometry: NaN coordinate in a referenced triangle"      # PT_ERR_SCENE
    assert flag.value == -5 and (cost == -7.0).all()
    same_records(records(r), before, "refused")
    same_image(frame(pt, r, 2), img, "refused")
    r.set_option("asm_node_layout", 1)                                    # a rebuild: the settled copies are the last accepted pose's, morph included
    got_img = frame(pt, r, 2)
    want, ref = fresh_records(pt, renderer_mod, new1, MC.SKY, (MC.W, MC.H), asm_node_layout=1)
    same_records(records(r), want, "the settled copies")
    same_image(got_img, ref, "the settled copies")
    pose.morph_weights(ws[1])                                             # and the pose is still usable
    assert r.pose_geometry(pose, X)[1] is True
    new2 = dict(old)
    new2[3], new2[10] = MC.move_of(old, MM.morph_skin(old[3], targets, ws[1], bone, weight, X))
    got_img = frame(pt, r, 2)
    want, ref = fresh_records(pt, renderer_mod, new2, MC.SKY, (MC.W, MC.H), asm_node_layout=1)
    same_records(records(r), want, "a good pose after the refusal")
    same_image(got_img, ref, "a good pose after the refusal")
    pose.close(); r.close()


def test_a_refusal_after_a_pose_accepted_before_the_attach_restores_it_unmorphed(pt, renderer_mod, soup):
    old, bone, weight, targets, X, ws = soup
    new1 = dict(old)
    new1[3], new1[10] = MC.move_of(old, SM.skin(old[3], bone, weight, X))
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H), asm_node_layout=0)
    frame(pt, r, 1)
    pose = r.skin_create(bone, weight, 3)
    assert r.pose_geometry(pose, X)[1] is True                           # accepted before the attach: counts as accepted with every weight 0
    attach(pose, targets)
    pose.morph_weights(np.array([0.0, 0.0, 0.0, 0.0, 3e38], f32))
    with pytest.raises(renderer_mod.PtError) as e:
        r.pose_geometry(pose, X)
    assert e.value.code == -4 and "NaN coordinate in a referenced triangle" in str(e.value)
    r.set_option("asm_node_layout", 1)
    got_img = frame(pt, r, 2)
    want, ref = fresh_records(pt, renderer_mod, new1, MC.SKY, (MC.W, MC.H), asm_node_layout=1)
    same_records(records(r), want, "the settled copies")
    same_image(got_img, ref, "the settled copies")
    pose.close(); r.close()


# ------------------------------------------------------------------------------------------------ staleness, a second attach, attach-time refusals

def test_staleness_a_second_attach_and_the_refusals_that_need_a_pose(pt, renderer_mod, soup):
    old, bone, weight, targets, X, ws = soup
    n = old[3].size // 40
    PtError = renderer_mod.PtError
    r = context(renderer_mod, old, MC.SKY, (MC.W, MC.H))
    frame(pt, r, 1)

    def refused(call, code, text):
        with pytest.raises(PtError) as e:
            call()
        assert e.value.code == code and text in str(e.value), str(e.value)

    D = np.zeros((1, 6), f32)
    # a static corner, on both kinds of pose
    skin = r.skin_create(bone, weight, 3)
    q_static = int(np.nonzero(bone.reshape(-1, 4)[:, 0] < 0)[0][0])
    q_moved = int(MM.moved_corners(n, bone=bone)[0])
    refused(lambda: skin.morph_attach([(np.array([q_moved, q_static], np.int32), np.tile(D, (2, 1)))]), -1, "pt_morph_attach: a corner that the pose's rule leaves static")
    parts = PM.parts_mod4(n)
    part = r.pose_create(parts, 3)
    refused(lambda: part.morph_attach([(np.array([3 * 1, 3 * 0 + 2], np.int32), np.tile(D, (2, 1)))]), -1, "pt_morph_attach: a corner that the pose's rule leaves static")
    refused(lambda: part.morph_attach([(np.array([3 * n], np.int32), D)]), -1, "pt_morph_attach: a corner outside [0, 3 * n_tris)")
    refused(lambda: part.morph_weights(np.zeros(1, f32)), -1, "pt_morph_weights: the pose has no morph")      # a refused attach attached nothing
    none = r.pose_create(np.full(n, -1, np.int32), 0)
    refused(lambda: none.morph_attach([(np.array([0], np.int32), D)]), -1, "pt_morph_attach: a corner that the pose's rule leaves static")      # n_parts == 0: one entry
    none.morph_attach([(np.zeros(0, np.int32), np.zeros((0, 6), f32))])                                       # ... and none: accepted
    none.morph_weights(np.array([2.0], f32))
    same_bits(none.triangles(np.zeros(0, f32)), old[3], "n_parts = 0: the rest pose")
    # a second attach; the weights' own refusals
    attach(skin, targets)
    refused(lambda: skin.morph_attach(targets), -1, "pt_morph_attach: the pose has a morph already")
    refused(lambda: skin.morph_weights(np.zeros(4, f32)), -1, "pt_morph_weights: weight_bytes != n_targets * 4")
    refused(lambda: skin.morph_weights(np.array([0, 0, np.inf, 0, 0], f32)), -1, "pt_morph_weights: a weight that is not finite")
    skin.morph_weights(ws[0])
    assert r.pose_geometry(skin, X)[1] is True
    # stale after an upload of binding 3
    r.set_buffer(3, old[3])
    refused(lambda: r.pose_geometry(skin, X), -4, "the scene was uploaded since pt_pose_create")
    refused(lambda: part.morph_attach([(np.array([3], np.int32), D)]), -4, "the scene was uploaded since pt_pose_create")
    again = attach(r.skin_create(bone, weight, 3), targets)              # a new morphed pose over the uploaded scene works
    again.morph_weights(ws[0])
    assert r.pose_geometry(again, X)[1] is True
    frame(pt, r, 2)
    new = dict(old)
    new[3], new[10] = MC.move_of(old, MM.morph_skin(old[3], targets, ws[0], bone, weight, X))
    same_records(records(r), fresh_records(pt, renderer_mod, new, MC.SKY, (MC.W, MC.H))[0], "a new morphed pose after the upload")
    r.close()


# ------------------------------------------------------------------------------------------------ the slow path

def test_slow_path_multi_stream_context(pt, renderer_mod, m4):
    rest, old, tex, bone, weight, targets, steps = m4
    X, w = steps[1]
    new = dict(old)
    new[3], new[10] = MC.move_of(old, MM.morph_skin(old[3], targets, w, bone, weight, X))
    r = renderer_mod.Renderer(rest.W, rest.H, devices=[0, 0])
    r.load_workload(rest)
    frame(pt, r, 1)
    pose = attach(r.skin_create(bone, weight, 5), targets)
    pose.morph_weights(w)
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
