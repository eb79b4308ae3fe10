"""GPU: include/pt_rig.h — pt_rig_records and pt_rig_clip_records against the numpy model of the rule (tests/_rig_model.py) bit for bit, and
pt_rig_pose_geometry / pt_rig_clip_pose_geometry against a twin context on which pt_pose_geometry ran with the downloaded records: every device
record array byte for byte, the next frame, root_cost and in_place; the refusal of a NaN local and what a later settle delivers; staleness, the
multi-stream slow path, destroyed rigs and poses.  96 x 54 or 48 x 27, a frame or two; the hierarchies are the smallest at which the launches
can go wrong: one joint, two, a chain with more levels than a wave has lanes, a level wider than a block and no multiple of 64, a forest of
1000 joints over some sixty levels with roots at the end of the table, the deepest chain allowed, no joint at all.

A NaN the rule generates (0 / 0 under a zero scale) equals any NaN: its sign and payload are the hardware's, and the model runs on another.
Everything else, the infinities included, is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _move_cases as MC
import _pose_model as PM
import _rig_model as RM
from test_gpu_move import context, frame, records, same_image, same_records
from test_gpu_pose import one_soup, same_floats
from test_rig_rule import clip_cases, rule_cases

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN_TEXT = "NaN coordinate in a referenced triangle"


def make_rig(pose, parent, bind=None):
    assert hasattr(pose._L, "pt_rig_create") and hasattr(pose, "rig")      # never skipped: a library without the symbol fails here
    return pose.rig(parent, bind)


@pytest.fixture(scope="module")
def bench(pt, renderer_mod):
    """a context over a soup of 4 triangles, all static: poses of any n_parts for the rule alone"""
    b = one_soup(pt, 4)
    r = context(renderer_mod, b, MC.SKY, (MC.W, MC.H))
    yield r, np.full(4, -1, np.int32)
    r.close()


# ------------------------------------------------------------------------------------------------ the rule alone

RULE_CASES = rule_cases()


@pytest.mark.parametrize("k", range(len(RULE_CASES)), ids=["-".join(c[0]) for c in RULE_CASES])
def test_rig_records_equal_the_model_bit_for_bit(bench, k):
    r, static = bench
    tag, parent, l, bind = RULE_CASES[k]
    n = parent.size
    pose = r.pose_create(static, n)
    rig = make_rig(pose, parent, bind)
    want = RM.records(parent, l, bind)
    got = rig.records(l)
    same_floats(got, want, tag)
    if tag[1] == "zero scale":
        assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(np.isnan(got), np.isnan(want))
        if bind is None:                                                   # M is W, whose column 0 is exactly zero at the scaled joint: c / 0 and 0 / 0
            assert np.isinf(want[n // 2, 12:21]).any() and np.isnan(want[n // 2, 12:21]).any()
    if n:                                                                  # the timed launches write the same records, and the call changes nothing of the pose
        x = np.ascontiguousarray(l, f32).reshape(-1)
        best = C.c_float(-1.0)
        assert r._L.pt_debug_rig_time(rig._h, x.ctypes.data, x.nbytes, 2, C.byref(best)) == 0, r._L.pt_last_error()
        assert best.value >= 0.0
        same_floats(rig.records(l), want, (tag, "again"))
    other = RM.random_locals(n, 99)                                        # a second evaluation on the same rig: nothing is left over from the first
    same_floats(rig.records(other), RM.records(parent, other, bind), (tag, "other locals"))
    rig.close(); pose.close()


def test_two_rigs_on_one_pose_do_not_meet(bench):
    r, static = bench
    pose = r.pose_create(static, 65)
    a, b = make_rig(pose, RM.chain(65)), make_rig(pose, RM.star(64), RM.random_binds(65, 1))
    l = RM.case_locals("chain65", 65)
    want_a, want_b = RM.records(RM.chain(65), l), RM.records(RM.star(64), l, RM.random_binds(65, 1))
    same_floats(a.records(l), want_a, "a"); same_floats(b.records(l), want_b, "b"); same_floats(a.records(l), want_a, "a again")
    assert not np.array_equal(want_a, want_b)
    a.close(); b.close(); pose.close()


# ------------------------------------------------------------------------------------------------ the clip

def test_clip_records_equal_the_model_at_between_before_and_after_the_keys(bench, renderer_mod):
    r, static = bench
    cases = clip_cases()
    rigs, seen = {}, set()
    for tag, parent, bind, times, values, t in cases:
        key = (tag[0], times.size)
        if key not in rigs:
            pose = r.pose_create(static, parent.size)
            rigs[key] = (pose, make_rig(pose, parent, bind))
            rigs[key][1].clip(times, values)
        rig = rigs[key][1]
        got = rig.records_at(t)
        same_floats(got, RM.clip_records(parent, times, values, t, bind), tag)
        exact, k, u = RM.interval(times, t)
        if exact >= 0 and parent.size:                                     # at a key, and clamped: that key's own records, bit for bit
            same_floats(got, rig.records(values.reshape(times.size, -1, 12)[exact]), (tag, "the key's own"))
            seen.add((tag[0], exact))
        elif parent.size:
            seen.add((tag[0], "between", bool(RM.flips(values[k], values[k + 1]).all())))
    assert {("forest40", 0), ("forest40", 1), ("forest40", 2), ("forest40", 3), ("one key", 0), ("forest40", "between", True), ("forest40", "between", False)} <= seen
    # a replaced clip: the second attach's keys answer, the first's are gone
    tag, parent, bind, times, values, _ = cases[0]
    rig = rigs[("forest40", 4)][1]
    times2, values2 = np.array([1.0, 3.0], f32), np.stack([RM.random_locals(40, 70), RM.random_locals(40, 71)])
    rig.clip(times2, values2)
    for t in (0.25, 1.0, 2.5, 3.0, 4.0):
        same_floats(rig.records_at(t), RM.clip_records(parent, times2, values2, t, bind), ("replaced", t))
    assert not np.array_equal(RM.clip_records(parent, times2, values2, 2.5, bind), RM.clip_records(parent, times, values, 2.5, bind))
    with pytest.raises(renderer_mod.PtError) as e:
        rig.records_at(np.nan)
    assert e.value.code == -1 and str(e.value).endswith("pt_rig_clip_records: t is NaN")
    for pose, rg in rigs.values():
        rg.close(); pose.close()


def test_a_rig_without_a_clip_refuses_a_time(bench, renderer_mod):
    r, static = bench
    pose = r.pose_create(static, 2)
    rig = make_rig(pose, RM.chain(2))
    with pytest.raises(renderer_mod.PtError) as e:
        rig.records_at(0.5)
    assert e.value.code == -1 and str(e.value).endswith("pt_rig_clip_records: no clip attached")
    with pytest.raises(renderer_mod.PtError) as e:
        rig.pose_at(0.5)
    assert e.value.code == -1 and str(e.value).endswith("pt_rig_clip_pose_geometry: no clip attached")
    rig.close(); pose.close()


# ------------------------------------------------------------------------------------------------ equivalence with pt_pose_geometry on a twin

def m1_case(pt):
    """M1 under the part rule: the box hangs on the room's (static) frame as a root, the sphere is the box's child, the poster a second root"""
    rest = pt.scenes.m1_moving(0)
    old, tex = MC.workload_inputs(rest)
    n = old[3].size // 40
    parts = np.full(n, -1, np.int32)
    parts[n - 334:n - 322] = 0; parts[n - 322:n - 2] = 1; parts[n - 2:] = 2
    parent = np.array([-1, 0, -1], np.int32)
    keys = []
    for s in (0.0, 2.0, 4.0):
        l = np.zeros((3, 12), f32)
        l[:, 7] = 1.0; l[:, 8:11] = 1.0
        l[0, 0:3] = (0.02 * s, 0.0, -0.01 * s); l[0, 5], l[0, 7] = np.sin(0.01 * s), np.cos(0.01 * s)
        l[1, 5], l[1, 7] = np.sin(0.015 * s), np.cos(0.015 * s)
        l[2, 0] = 0.015 * s
        keys.append(l)
    return dict(rest=rest, old=old, tex=tex, make=lambda r: r.pose_create(parts, 3), parent=parent, bind=None, times=np.array([0.0, 1.0, 2.0], f32), values=np.stack(keys))


def m7_case(pt, blend, chained=False):
    """M7 (M3's tube as one chain) under the linear or the dual-quaternion skin; chained: M5's morph ahead and recomputed normals behind"""
    wl, bone, weight, parent, bind, times, values = pt.scenes.m7_chained()
    old, tex = MC.workload_inputs(wl)

    def make(r):
        pose = r.skin_create(bone, weight, 5, blend=blend)
        if chained:
            _, _, _, targets, _, w4, ids, nv = pt.scenes.m5_rippling(3)
            pose.morph_attach(targets); pose.normals_attach(ids, nv); pose.morph_weights(w4)
            assert (w4 != 0).any()
        return pose
    return dict(rest=wl, old=old, tex=tex, make=make, parent=parent, bind=bind, times=times, values=values)


def _run(pt, renderer_mod, case, how, what, **opts):
    """one context: a frame, the step, the records at once, the next frame, the records after it.  how: "rig" (locals), "clip" (a time) or
    "twin" (pt_pose_geometry with the records `what`)"""
    r = context(renderer_mod, case["old"], case["tex"], (case["rest"].W, case["rest"].H), **opts)
    frame(pt, r, 1)
    pose = case["make"](r)
    rig = make_rig(pose, case["parent"], case["bind"])
    rig.clip(case["times"], case["values"])
    if how == "rig":
        R = rig.records(what)
        cost, in_place = rig.pose(what)
    elif how == "clip":
        R = rig.records_at(what)
        cost, in_place = rig.pose_at(what)
    else:
        R = what
        cost, in_place = r.pose_geometry(pose, what)
    out = (cost, in_place, records(r, skip=("ellip",)), frame(pt, r, 2), records(r), R)
    rig.close(); pose.close(); r.close()
    return out


def _same_as_twin(pt, renderer_mod, case, how, what, tag, **opts):
    cost, flag, at_once, img, after, R = _run(pt, renderer_mod, case, how, what, **opts)
    model = RM.records(case["parent"], what, case["bind"]) if how == "rig" else RM.clip_records(case["parent"], case["times"], case["values"], what, case["bind"])
    same_floats(R, model, (tag, "the records"))
    cost2, flag2, at_once2, img2, after2, _ = _run(pt, renderer_mod, case, "twin", R, **opts)
    assert flag is True and flag2 is True, (tag, flag, flag2)                # in_place, and equal
    assert np.array_equal(cost.view(np.uint64), cost2.view(np.uint64)) and cost.size == int(case["old"][13][0]), tag      # root_cost
    same_records(at_once, at_once2, (tag, "before the next render"))
    same_records(after, after2, tag)
    same_image(img, img2, tag)
    return after


@pytest.mark.parametrize("name", ["parts", "skin", "dq", "chained"])
def test_rig_pose_geometry_equals_pose_geometry_of_the_downloaded_records(pt, renderer_mod, name):
    case = m1_case(pt) if name == "parts" else m7_case(pt, "dq" if name == "dq" else "linear", chained=name == "chained")
    moved = _same_as_twin(pt, renderer_mod, case, "rig", case["values"][1], (name, "locals"))
    rest = _same_as_twin(pt, renderer_mod, case, "rig", case["values"][0], (name, "rest locals"))
    assert not np.array_equal(moved["tris"], rest["tris"])                   # the pose did move something
    t = 0.5 * float(case["times"][1] + case["times"][2])
    between = _same_as_twin(pt, renderer_mod, case, "clip", t, (name, "clip", t))
    assert not np.array_equal(between["tris"], moved["tris"])
    at_key = _same_as_twin(pt, renderer_mod, case, "clip", float(case["times"][1]), (name, "clip at key 1"))
    same_records(at_key, moved, (name, "the clip at a key is that key's locals"))


def test_rig_pose_geometry_under_bfs3(pt, renderer_mod):
    _same_as_twin(pt, renderer_mod, m7_case(pt, "linear"), "rig", m7_case(pt, "linear")["values"][2], ("skin", "bfs3"), bfs_nodes=3)


# ------------------------------------------------------------------------------------------------ refusal and restore

def test_a_nan_local_is_refused_and_a_later_settle_delivers_the_last_accepted_pose(pt, renderer_mod):
    case = m7_case(pt, "linear")
    L = renderer_mod.lib()
    good, bad = case["values"][1], case["values"][2].copy()
    bad[3, 0] = np.nan                                                      # joint 3's translation: its records and its child's hold NaN
    assert np.isnan(RM.records(case["parent"], bad, case["bind"])[3:, :12]).any()
    size = (case["rest"].W, case["rest"].H)
    r = context(renderer_mod, case["old"], case["tex"], size, asm_node_layout=0)
    frame(pt, r, 1)
    pose = case["make"](r)
    rig = make_rig(pose, case["parent"], case["bind"])
    rig.clip(case["times"], np.stack([case["values"][0], bad, case["values"][2]]))

    def refused(call, name):
        flag, cost = C.c_int(-5), np.full(pose.n_roots, -7.0)
        rc = call(cost.ctypes.data, C.byref(flag))
        assert rc == -4 and L.pt_last_error().decode() == f"{name}: {NAN_TEXT}"      # PT_ERR_SCENE: the refusal of every NaN coordinate, under the call's name
        assert flag.value == -5 and (cost == -7.0).all()

    x = np.ascontiguousarray(bad, f32).reshape(-1)
    by_locals = lambda cost, flag: L.pt_rig_pose_geometry(r._h, rig._h, x.ctypes.data, x.nbytes, None, 0, cost, flag)
    by_clip = lambda cost, flag: L.pt_rig_clip_pose_geometry(r._h, rig._h, float(case["times"][1]), None, 0, cost, flag)
    img0, before0 = frame(pt, r, 2), records(r)
    refused(by_locals, "pt_rig_pose_geometry")                              # no accepted pose yet: the rest pose stays
    same_records(records(r), before0, "refused first")
    same_image(frame(pt, r, 2), img0, "refused first")
    assert rig.pose(good)[1] is True                                        # the rig is still usable
    R = rig.records(good)
    img, before = frame(pt, r, 2), records(r)
    refused(by_locals, "pt_rig_pose_geometry")
    refused(by_clip, "pt_rig_clip_pose_geometry")
    same_records(records(r), before, "refused")
    same_image(frame(pt, r, 2), img, "refused")
    r.set_option("asm_node_layout", 1)                                      # a rebuild: the settled copies are the last accepted pose's
    got_img = frame(pt, r, 2)
    got = records(r)
    rig.close(); pose.close(); r.close()
    twin = context(renderer_mod, case["old"], case["tex"], size, asm_node_layout=0)      # the same history through pt_pose_geometry
    frame(pt, twin, 1)
    pose = case["make"](twin)
    assert twin.pose_geometry(pose, R)[1] is True
    frame(pt, twin, 2)
    twin.set_option("asm_node_layout", 1)
    want_img = frame(pt, twin, 2)
    same_records(got, records(twin), "the settled copies")
    same_image(got_img, want_img, "the settled copies")
    pose.close(); twin.close()


# ------------------------------------------------------------------------------------------------ other paths

def test_a_stale_pose_is_refused_under_the_rig_s_name(pt, renderer_mod):
    case = m7_case(pt, "linear")
    r = context(renderer_mod, case["old"], case["tex"], (case["rest"].W, case["rest"].H))
    frame(pt, r, 1)
    pose = case["make"](r)
    rig = make_rig(pose, case["parent"], case["bind"])
    rig.clip(case["times"], case["values"])
    assert rig.pose(case["values"][1])[1] is True
    r.set_buffer(3, case["old"][3])
    for call, name in ((lambda: rig.pose(case["values"][1]), "pt_rig_pose_geometry"), (lambda: rig.pose_at(1.0), "pt_rig_clip_pose_geometry")):
        with pytest.raises(renderer_mod.PtError) as e:
            call()
        assert e.value.code == -4 and str(e.value).endswith(f"{name}: the scene was uploaded since pt_pose_create")
    same_floats(rig.records(case["values"][1]), RM.records(case["parent"], case["values"][1], case["bind"]), "the rule alone still answers")
    r.close()


def test_a_rig_of_another_context_is_refused(pt, renderer_mod, bench):
    r, static = bench
    pose = r.pose_create(static, 2)
    rig = make_rig(pose, RM.chain(2))
    rig.clip(np.array([0.0], f32), RM.random_locals(2, 1))
    other = context(renderer_mod, one_soup(pt, 4), MC.SKY, (MC.W, MC.H))
    L = renderer_mod.lib()
    x = RM.random_locals(2, 1).reshape(-1)
    assert L.pt_rig_pose_geometry(other._h, rig._h, x.ctypes.data, x.nbytes, None, 0, None, None) == -1
    assert L.pt_last_error().decode() == "pt_rig_pose_geometry: the rig's pose was created on another context"
    assert L.pt_rig_clip_pose_geometry(other._h, rig._h, 0.0, None, 0, None, None) == -1
    assert L.pt_last_error().decode() == "pt_rig_clip_pose_geometry: the rig's pose was created on another context"
    other.close(); rig.close(); pose.close()


def test_slow_path_multi_stream_context(pt, renderer_mod):
    case = m7_case(pt, "linear")
    rest = case["rest"]
    l = case["values"][1]
    r = renderer_mod.Renderer(rest.W, rest.H, devices=[0, 0])
    r.load_workload(rest)
    frame(pt, r, 1)
    pose = case["make"](r)
    rig = make_rig(pose, case["parent"], case["bind"])
    R = rig.records(l)
    same_floats(R, RM.records(case["parent"], l, case["bind"]), "multi")
    cost, in_place = rig.pose(l)
    assert in_place is False
    img = frame(pt, r, 2)
    rig.close(); pose.close(); r.close()
    single = context(renderer_mod, case["old"], case["tex"], (rest.W, rest.H))      # a fresh single-stream context's frame of the same pose
    frame(pt, single, 1)
    one = case["make"](single)
    cost1, flag = single.pose_geometry(one, R)
    assert flag is True and np.array_equal(cost.view(np.uint64), cost1.view(np.uint64))
    ref = frame(pt, single, 2)
    one.close(); single.close()
    same_image(img, ref, "multi")


def test_destroyed_rigs_and_rigs_of_destroyed_poses_are_refused(pt, renderer_mod, bench):
    r, static = bench
    L = renderer_mod.lib()
    l = RM.random_locals(3, 5)
    x, out = l.reshape(-1), np.zeros(72, f32)

    def refused(h):
        assert L.pt_rig_records(h, x.ctypes.data, x.nbytes, out.ctypes.data, out.nbytes) == -1 and L.pt_last_error().decode() == "pt_rig_records: null or destroyed rig"
        assert L.pt_rig_pose_geometry(r._h, h, x.ctypes.data, x.nbytes, None, 0, None, None) == -1
        assert L.pt_last_error().decode() == "pt_rig_pose_geometry: null or destroyed rig"
        assert L.pt_rig_clip_attach(h, 1, x.ctypes.data, 4, x.ctypes.data, x.nbytes) == -1 and L.pt_last_error().decode() == "pt_rig_clip_attach: null or destroyed rig"
        L.pt_rig_destroy(h)                                                 # a second destroy is not followed either

    pose = r.pose_create(static, 3)
    rig, keep = make_rig(pose, RM.star(2)), make_rig(pose, RM.chain(3))
    h = C.c_void_p(rig._h.value)
    rig.close()
    refused(h)
    same_floats(keep.records(l), RM.records(RM.chain(3), l), "the pose's other rig lives on")
    h = C.c_void_p(keep._h.value)
    pose.close()                                                            # pt_pose_destroy destroys the pose's rigs
    refused(h)
    keep._h = None
    out2 = C.c_void_p(0)
    parent = RM.chain(3)
    ctx = context(renderer_mod, one_soup(pt, 4), MC.SKY, (MC.W, MC.H))     # pt_destroy destroys the poses' rigs
    p2 = ctx.pose_create(static, 3)
    g2 = make_rig(p2, RM.chain(3))
    h2, hp = C.c_void_p(g2._h.value), C.c_void_p(p2._h.value)
    ctx.close()
    refused(h2)
    assert L.pt_rig_create(hp, parent.ctypes.data, parent.nbytes, None, 0, C.byref(out2)) == -1 and L.pt_last_error().decode() == "pt_rig_create: the pose is not live"
    g2._h = None; p2._h = None


# ------------------------------------------------------------------------------------------------ the timers' argument checks

def test_every_timer_of_the_family_refuses_under_its_own_name(pt, renderer_mod):
    """The seven pt_debug_*_time calls of the pose family share their argument checks: each one, with one argument wrong at a time (a null
    msBest, reps == 0, null data, a byte count off by 4, a destroyed handle), answers -1 and "<name>: bad argument" before anything is
    enqueued, leaves *msBest alone, and times a good call afterwards.  Two triangles, one moving; one part, one joint."""
    L = renderer_mod.lib()
    r = context(renderer_mod, one_soup(pt, 2), MC.SKY, (MC.W, MC.H))
    bone, weight = np.full((2, 12), -1, np.int32), np.zeros((2, 12), f32)
    bone[0, 0::4], weight[0, 0::4] = 0, 1.0
    parts = np.array([0, -1], np.int32)
    part, skin, dq = r.pose_create(parts, 1), r.skin_create(bone, weight, 1), r.skin_create(bone, weight, 1, blend="dq")
    part.morph_attach([(np.array([0], np.int32), np.full((1, 6), 0.25, f32))])
    part.normals_attach(np.array([0, 1, 2, -1, -1, -1], np.int32))
    rig = make_rig(part, RM.chain(1))
    rig.mix_clip(0, np.array([0.0], f32), RM.random_locals(1, 1))
    gone = r.pose_create(parts, 1)                                          # destroyed below, after the last create: its address is not handed out again
    gone_rig = make_rig(gone, RM.chain(1))
    dead, dead_rig = C.c_void_p(gone._h.value), C.c_void_p(gone_rig._h.value)
    gone.close(); gone_rig._h = None                                        # the rig went with its pose
    x = np.ascontiguousarray(PM.matrices(1), f32).reshape(-1)
    w = np.array([0.5], f32)
    l = np.ascontiguousarray(RM.random_locals(1, 2), f32).reshape(-1)
    y = renderer_mod.rig_layers([(0, 0.0)])
    assert (x.nbytes, w.nbytes, l.nbytes, y.nbytes) == (96, 4, 48, 24)
    # (the call, its handle, a destroyed one, the data, the arguments between the byte count and reps)
    timers = [("pt_debug_pose_time", part._h, dead, x, (0,)), ("pt_debug_skin_time", skin._h, dead, x, (0,)), ("pt_debug_skin_dq_time", dq._h, dead, x, ()),
              ("pt_debug_normals_time", part._h, dead, x, (0,)), ("pt_debug_morph_time", part._h, dead, w, ()), ("pt_debug_rig_time", rig._h, dead_rig, l, ()),
              ("pt_debug_rig_mix_time", rig._h, dead_rig, y, ())]
    for name, h, destroyed, data, which in timers:
        call, best = getattr(L, name), C.c_float(-2.0)
        p, nb, ms = data.ctypes.data, data.nbytes, C.byref(best)
        bad = {"null msBest": (h, p, nb, *which, 1, None), "reps == 0": (h, p, nb, *which, 0, ms), "null data": (h, None, nb, *which, 1, ms),
               "four bytes more": (h, p, nb + 4, *which, 1, ms), "four bytes less": (h, p, nb - 4, *which, 1, ms), "destroyed": (destroyed, p, nb, *which, 1, ms)}
        for what, args in bad.items():
            assert call(*args) == -1, (name, what)
            assert L.pt_last_error().decode() == f"{name}: bad argument", (name, what, L.pt_last_error())
            assert best.value == -2.0, (name, what)
        assert call(h, p, nb, *which, 1, ms) == 0, (name, L.pt_last_error())
        assert best.value >= 0.0, name
    r.close()
