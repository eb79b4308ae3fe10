"""GPU: include/pt_rig_ik.h — pt_rig_ik_locals against the numpy model of the rule (tests/_rig_ik_model.py) bit for bit on the cases the C++
check runs; every record call of a rig with goals set against pt_rig_records, goals off, of the downloaded pt_rig_ik_locals of that call's
source's locals; the three geometry calls against a twin context on which pt_pose_geometry ran with the model's records: every device record
array byte for byte, the next frame, root_cost and in_place, under the part, skin and dual-quaternion rules; goals off again, a replaced table,
two rigs on one pose, the refusals of a live rig in the header's order, destroyed rigs, staleness, the timer.  The rigs are the smallest at which
the launch and the level window can go wrong: a chain at the rig's root, one under a parent, first joints at two depths, 65 constraints, none.

A NaN the rule generates equals any NaN: its sign and payload are the hardware's.  Everything else is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _move_cases as MC
import _rig_ik_model as IM
import _rig_mix_model as MM
import _rig_model as RM
from test_gpu_move import context, frame, records, same_image, same_records
from test_gpu_pose import one_soup, same_floats
from test_gpu_rig import _run, m1_case, make_rig
from test_gpu_rig_mix import fill, m8_case, pack

pytestmark = pytest.mark.gpu

f32 = np.float32


def attach(rig, cons, goals):
    assert hasattr(rig._L, "pt_rig_ik_attach") and hasattr(rig, "ik")       # never skipped: a library without the symbol fails here
    rig.ik(IM.pack_constraints(cons))
    rig.ik_goals(None if goals is None else IM.pack_goals(goals))


@pytest.fixture(scope="module")
def bench(pt, renderer_mod):
    """a context over a soup of 4 triangles, all static: poses of any n_parts for the rule alone"""
    b = one_soup(pt, 4)
    r = context(renderer_mod, b, MC.SKY, (MC.W, MC.H))
    yield r, np.full(4, -1, np.int32)
    r.close()


# ------------------------------------------------------------------------------------------------ the rule alone

IK_CASES = IM.ik_cases()


@pytest.mark.parametrize("k", range(len(IK_CASES)), ids=[c["tag"].replace(" ", "_") for c in IK_CASES])
def test_ik_locals_equal_the_model_bit_for_bit(bench, k):
    r, static = bench
    case = IK_CASES[k]
    parent, l, cons, goals, bind = case["parent"], case["locals"], case["cons"], case["goals"], case["bind"]
    n = parent.size
    pose = r.pose_create(static, n)
    rig = make_rig(pose, parent, bind)
    attach(rig, cons, goals)
    want = IM.ik_locals(parent, cons, goals, l)
    got = rig.ik_locals(l)
    same_floats(got, want, case["tag"])
    keep = np.ones(12, bool); keep[4:8] = False
    assert np.array_equal(got[:, keep].view(np.uint32), l[:, keep].view(np.uint32))      # translations, scales and padding are never written
    rec = rig.records(l)                                                    # the levels around the solve, the window included
    same_floats(rec, RM.records(parent, want, bind), (case["tag"], "the records"))
    if goals is not None and cons:                                          # the timed launch writes the same locals, and a following call answers the same
        best = C.c_float(-1.0)
        assert r._L.pt_debug_rig_ik_time(rig._h, l.ctypes.data, l.nbytes, 2, C.byref(best)) == 0, r._L.pt_last_error()
        assert best.value >= 0.0
        same_floats(rig.ik_locals(l), want, (case["tag"], "again"))
    rig.ik_goals(None)                                                      # goals off again: the goal-free answer
    assert np.array_equal(rig.ik_locals(l).view(np.uint32), l.view(np.uint32))
    same_floats(rig.records(l), RM.records(parent, l, bind), (case["tag"], "goals off"))
    if goals is not None:
        rig.ik_goals(IM.pack_goals(goals))
        same_floats(rig.records(l), rec, (case["tag"], "and on again"))
    rig.close(); pose.close()


def humanoid(seed=0):
    """the mixed table of _rig_ik_model.ik_cases on its humanoid, with a clip of three keys, two mix slots and a mask"""
    case = dict(next(c for c in IK_CASES if c["tag"] == "mixed kinds"))
    n = case["parent"].size
    times = np.array([0.0, 1.0, 2.5], f32)
    values = np.stack([case["locals"]] + [IM.rigid_locals(n, seed + 70 + k) for k in range(2)])
    clips = {0: (np.array([0.5, 2.0], f32), np.stack([IM.rigid_locals(n, seed + 80 + k) for k in range(2)])), 1: (times, values)}
    masks = {0: MM.ramp(n)}
    layers = [MM.layer(1, 1.5), MM.layer(0, 1.0, 0.75, 0), MM.layer(1, 0.5, 0.5, -1, MM.ADDITIVE)]
    case.update(times=times, values=values, clips=clips, masks=masks, layers=layers)
    return case


def test_every_record_call_with_goals_equals_the_records_of_ik_locals_of_its_source(bench, renderer_mod):
    """the caller's locals, the clip at a key (in place: copied first), the clip between keys and the mix, in any order; a clip's keys are
    never written; pt_rig_mix_locals stays the mix alone"""
    r, static = bench
    case = humanoid()
    parent, bind, cons, goals, times, values, clips, masks, layers = (case[k] for k in ("parent", "bind", "cons", "goals", "times", "values", "clips", "masks", "layers"))
    n = parent.size
    pose = r.pose_create(static, n)
    rig = make_rig(pose, parent, bind)
    rig.clip(times, values)
    fill(rig, clips, masks)
    y = pack(renderer_mod, layers)
    A = IM.rigid_locals(n, 99)
    assert RM.interval(times, f32(1.0))[0] == 1 and RM.interval(times, f32(1.75))[0] < 0
    sources = [("records(A)", lambda: rig.records(A), A), ("records_at(key 1)", lambda: rig.records_at(1.0), values[1]),
               ("records_at(between keys)", lambda: rig.records_at(1.75), RM.clip_locals(times, values, n, f32(1.75))),
               ("mix_records", lambda: rig.mix_records(y), MM.mix_locals(clips, masks, layers, n)), ("records_at(key 0)", lambda: rig.records_at(0.0), values[0])]
    free = [call() for _, call, _ in sources]                               # no table yet: the goal-free answers
    attach(rig, cons, goals)
    answers = []
    for tag, call, src in sources + sources[::-1]:
        got = call()
        solved = rig.ik_locals(src)                                         # downloaded
        same_floats(solved, IM.ik_locals(parent, cons, goals, src), (tag, "ik_locals of the source's locals"))
        rig.ik_goals(None)
        want = rig.records(solved)                                          # pt_rig_records, goals off
        rig.ik_goals(IM.pack_goals(goals))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), tag
        same_floats(got, IM.ik_records(parent, cons, goals, src, bind), (tag, "the model"))
        answers.append(got)
    assert len({a.tobytes() for a in answers}) == len(sources)              # five different answers, each the same in both orders
    same_floats(rig.mix_locals(y), MM.mix_locals(clips, masks, layers, n), "pt_rig_mix_locals stays the mix alone")
    zero = [IM.goal(g["target"], 0.0, g["pole"]) for g in goals]            # every weight 0: the goal-free answers, bit for bit
    rig.ik_goals(IM.pack_goals(zero))
    for (tag, call, _), was in zip(sources, free):
        assert np.array_equal(call().view(np.uint32), was.view(np.uint32)), (tag, "weights 0")
    rig.ik_goals(None)                                                      # goals off: likewise, and the clip's keys are what they were
    for (tag, call, _), was in zip(sources, free):
        assert np.array_equal(call().view(np.uint32), was.view(np.uint32)), (tag, "goals off")
    rig.close(); pose.close()


def test_an_attach_replaces_the_table_and_clears_the_goals(bench, renderer_mod):
    r, static = bench
    case = humanoid()
    parent, l, cons, goals = case["parent"], case["locals"], case["cons"], case["goals"]
    pose = r.pose_create(static, parent.size)
    rig = make_rig(pose, parent)
    attach(rig, cons, goals)
    same_floats(rig.ik_locals(l), IM.ik_locals(parent, cons, goals, l), "the first table")
    rig.ik(IM.pack_constraints(cons[:2]))                                   # goals cleared: the locals come back as given
    assert np.array_equal(rig.ik_locals(l).view(np.uint32), l.view(np.uint32))
    with pytest.raises(renderer_mod.PtError) as e:                                     # the old goals no longer fit
        rig.ik_goals(IM.pack_goals(goals))
    assert str(e.value).endswith("pt_rig_ik_goals: bytes != 32 * the table's constraints")
    rig.ik_goals(IM.pack_goals(goals[:2]))
    same_floats(rig.ik_locals(l), IM.ik_locals(parent, cons[:2], goals[:2], l), "the second table")
    with pytest.raises(renderer_mod.PtError) as e:                                     # a refused attach leaves table and goals as they were
        rig.ik(IM.pack_constraints([IM.two_bone(7), IM.aim(7, (0.0, 0.0, 1.0))]))
    assert str(e.value).endswith("pt_rig_ik_attach: constraint 0 reads a joint that another constraint writes")
    same_floats(rig.ik_locals(l), IM.ik_locals(parent, cons[:2], goals[:2], l), "after a refused attach")
    rig.ik([])                                                              # no table
    rig.ik_goals([])
    assert np.array_equal(rig.ik_locals(l).view(np.uint32), l.view(np.uint32))
    rig.close(); pose.close()


def test_two_rigs_on_one_pose_do_not_meet(bench):
    r, static = bench
    case = humanoid()
    parent, l, cons, goals = case["parent"], case["locals"], case["cons"], case["goals"]
    pose = r.pose_create(static, parent.size)
    a, b = make_rig(pose, parent), make_rig(pose, parent)
    other = [IM.goal(g["target"] + f32(0.25), g["weight"], g["pole"]) for g in goals]
    attach(a, cons, goals); attach(b, cons[:1], other[:1])
    want_a, want_b = IM.ik_locals(parent, cons, goals, l), IM.ik_locals(parent, cons[:1], other[:1], l)
    same_floats(a.ik_locals(l), want_a, "a"); same_floats(b.ik_locals(l), want_b, "b"); same_floats(a.ik_locals(l), want_a, "a again")
    b.ik_goals(None)
    same_floats(a.records(l), RM.records(parent, want_a), "a's goals stay"); same_floats(b.records(l), RM.records(parent, l), "b's are off")
    assert not np.array_equal(want_a, want_b)
    a.close(); b.close(); pose.close()


def test_a_live_rig_refuses_in_the_header_s_order(bench, renderer_mod):
    r, static = bench
    L = renderer_mod.lib()
    parent = IM.HUMANOID
    n = parent.size
    pose = r.pose_create(static, n)
    rig = make_rig(pose, parent)
    err = lambda: L.pt_last_error().decode()
    good = IM.pack_constraints([IM.two_bone(7, True), IM.aim(3, (0.0, 0.0, 1.0))])

    def attach_refused(c, nbytes, text, ptr=True):
        assert L.pt_rig_ik_attach(rig._h, c.ctypes.data if ptr else None, nbytes) == -1 and err() == "pt_rig_ik_attach: " + text, (text, err())
    attach_refused(good, 33, "bytes must be a multiple of 32")
    attach_refused(good, 64, "null constraints with bytes > 0", ptr=False)
    for field, value, k, text in (("kind", 2, 1, "unknown kind"), ("joint", n, 0, "a joint outside [0, n_parts)"), ("joint", 1, 0, "a tip without a parent and a grandparent"),
                                  ("flags", 2, 1, "flags other than 0 or PT_RIG_IK_POLE")):
        bad = good.copy()
        bad[field][k] = value
        attach_refused(bad, bad.nbytes, f"constraint {k}: {text}")
    bad = good.copy(); bad["flags"][0] = 4; bad["kind"][1] = 7              # constraint 0's later-listed fault answers before constraint 1's
    attach_refused(bad, bad.nbytes, "constraint 0: flags other than 0 or PT_RIG_IK_POLE")
    bad = good.copy(); bad["axis"][1] = (0.0, 0.0, 2.0)
    attach_refused(bad, bad.nbytes, "constraint 1: an axis that is not finite or not of length 1")
    bad = good.copy(); bad["joint"][1] = 2                                  # an aim on an ancestor of the chain
    attach_refused(bad, bad.nbytes, "constraint 0 reads a joint that another constraint writes")
    goals = IM.pack_goals([IM.goal((1.0, 1.0, 1.0)), IM.goal((0.0, 2.0, 0.0), 0.5)])
    assert L.pt_rig_ik_goals(rig._h, goals.ctypes.data, goals.nbytes) == -1 and err() == "pt_rig_ik_goals: bytes != 32 * the table's constraints"      # no table yet
    rig.ik(good)
    assert L.pt_rig_ik_goals(rig._h, None, 64) == -1 and err() == "pt_rig_ik_goals: null goals with bytes > 0"
    assert L.pt_rig_ik_goals(rig._h, goals.ctypes.data, 32) == -1 and err() == "pt_rig_ik_goals: bytes != 32 * the table's constraints"
    for w in (np.nan, -0.5, 1.5, np.inf):
        bad = goals.copy(); bad["weight"][1] = w
        assert L.pt_rig_ik_goals(rig._h, bad.ctypes.data, bad.nbytes) == -1 and err() == "pt_rig_ik_goals: goal 1: a weight must be finite and in [0, 1]"
    l, out = IM.rigid_locals(n, 3), np.zeros((n, 12), f32)
    for args, text in (((None, l.nbytes, out.ctypes.data, out.nbytes), "null locals with n_parts > 0"), ((l.ctypes.data, 48, out.ctypes.data, out.nbytes), "local_bytes != n_parts * 48"),
                       ((l.ctypes.data, l.nbytes, None, out.nbytes), "null locals_out"), ((l.ctypes.data, l.nbytes, out.ctypes.data, 48), "out_bytes != n_parts * 48")):
        assert L.pt_rig_ik_locals(rig._h, *args) == -1 and err() == "pt_rig_ik_locals: " + text
    assert not out.any()
    best = C.c_float(-2.0)                                                  # the timer: no goals set, then its arguments
    assert L.pt_debug_rig_ik_time(rig._h, l.ctypes.data, l.nbytes, 1, C.byref(best)) == -1 and err() == "pt_debug_rig_ik_time: bad argument"
    rig.ik_goals(goals)
    for args in ((None, l.nbytes, 1, C.byref(best)), (l.ctypes.data, 48, 1, C.byref(best)), (l.ctypes.data, l.nbytes, 0, C.byref(best)), (l.ctypes.data, l.nbytes, 1, None)):
        assert L.pt_debug_rig_ik_time(rig._h, *args) == -1 and err() == "pt_debug_rig_ik_time: bad argument"
    assert best.value == -2.0
    cons, gs = [IM.two_bone(7, True), IM.aim(3, (0.0, 0.0, 1.0))], [IM.goal((1.0, 1.0, 1.0)), IM.goal((0.0, 2.0, 0.0), 0.5)]
    same_floats(rig.ik_locals(l), IM.ik_locals(parent, cons, gs, l), "the rig still answers")
    rig.close(); pose.close()


def test_destroyed_rigs_and_rigs_of_destroyed_poses_are_refused(pt, renderer_mod, bench):
    r, static = bench
    L = renderer_mod.lib()
    parent = RM.chain(3)
    c, g = IM.pack_constraints([IM.two_bone(2)]), IM.pack_goals([IM.goal((0.5, 0.5, 0.5))])
    l, out, best = IM.rigid_locals(3, 1), np.zeros((3, 12), f32), C.c_float(-2.0)

    def refused(h):
        assert L.pt_rig_ik_attach(h, c.ctypes.data, c.nbytes) == -1 and L.pt_last_error().decode() == "pt_rig_ik_attach: null or destroyed rig"
        assert L.pt_rig_ik_goals(h, g.ctypes.data, g.nbytes) == -1 and L.pt_last_error().decode() == "pt_rig_ik_goals: null or destroyed rig"
        assert L.pt_rig_ik_locals(h, l.ctypes.data, l.nbytes, out.ctypes.data, out.nbytes) == -1 and L.pt_last_error().decode() == "pt_rig_ik_locals: null or destroyed rig"
        assert L.pt_debug_rig_ik_time(h, l.ctypes.data, l.nbytes, 1, C.byref(best)) == -1 and L.pt_last_error().decode() == "pt_debug_rig_ik_time: bad argument"

    pose = r.pose_create(static, 3)
    rig, keep = make_rig(pose, parent), make_rig(pose, parent)
    attach(rig, [IM.two_bone(2)], [IM.goal((0.5, 0.5, 0.5))]); attach(keep, [IM.two_bone(2)], [IM.goal((0.5, 0.5, 0.5))])
    h = C.c_void_p(rig._h.value)
    rig.close()                                                             # the table and the goals go with their rig
    refused(h)
    same_floats(keep.ik_locals(l), IM.ik_locals(parent, [IM.two_bone(2)], [IM.goal((0.5, 0.5, 0.5))], l), "the pose's other rig lives on")
    h = C.c_void_p(keep._h.value)
    pose.close()                                                            # pt_pose_destroy destroys the pose's rigs
    refused(h)
    keep._h = None
    assert not out.any() and best.value == -2.0


# ------------------------------------------------------------------------------------------------ equivalence with pt_pose_geometry on a twin

def m9_case(pt, renderer_mod, blend, step=3):
    """M9: M8 (m8_case) with joints 2-3-4 as a two-bone chain towards the step's goal"""
    case = m8_case(pt, renderer_mod, blend, step=step)
    m9 = pt.scenes.m9_reaching(step)
    y = m9[9][0]
    case.update(cons=[IM.two_bone(4, True)], goals=[IM.goal(y["target"], y["weight"], y["pole"])])
    assert renderer_mod.rig_ik_constraints(m9[8]).tobytes() == IM.pack_constraints(case["cons"]).tobytes()
    assert renderer_mod.rig_ik_goals(m9[9]).tobytes() == IM.pack_goals(case["goals"]).tobytes()
    return case


def _source(case, how):
    """(the call on a rig, the source's locals by the models)"""
    n = case["parent"].size
    if how == "locals":
        A = case["values"][1]
        return (lambda rig: rig.pose(A)), A
    if how == "clip at a key":
        assert RM.interval(case["times"], f32(1.0))[0] >= 0
        return (lambda rig: rig.pose_at(1.0)), RM.clip_locals(case["times"], case["values"], n, f32(1.0))
    return (lambda rig: rig.mix(case["layers"])), MM.mix_locals(case["clips"], case["masks"], case["model"], n)


def _ik_same_as_twin(pt, renderer_mod, case, how, tag, **opts):
    call, src = _source(case, how)
    want = IM.ik_records(case["parent"], case["cons"], case["goals"], src, case["bind"])      # the model's records
    assert not np.array_equal(want, RM.records(case["parent"], src, case["bind"])), tag      # the goal moves the pose
    r = context(renderer_mod, case["old"], case["tex"], (case["rest"].W, case["rest"].H), **opts)
    frame(pt, r, 1)
    pose = case["make"](r)
    rig = make_rig(pose, case["parent"], case["bind"])
    rig.clip(case["times"], case["values"])
    if "clips" in case:
        fill(rig, case["clips"], case["masks"])
    attach(rig, case["cons"], case["goals"])
    cost, flag = call(rig)
    at_once, img, after = records(r, skip=("ellip",)), frame(pt, r, 2), records(r)
    if how == "clip at a key":                                              # the clip's keys are unchanged afterwards
        rig.ik_goals(None)
        same_floats(rig.records_at(1.0), RM.clip_records(case["parent"], case["times"], case["values"], f32(1.0), case["bind"]), (tag, "the keys"))
    rig.close(); pose.close(); r.close()
    cost2, flag2, at_once2, img2, after2, _ = _run(pt, renderer_mod, case, "twin", want, **opts)      # pt_pose_geometry with the model's records
    assert flag is True and flag2 is True, (tag, flag, flag2)
    assert np.array_equal(cost.view(np.uint64), cost2.view(np.uint64)), tag
    same_records(at_once, at_once2, (tag, "before the next render"))
    same_records(after, after2, tag)
    same_image(img, img2, tag)


@pytest.mark.parametrize("how", ["locals", "clip at a key", "mix"])
def test_the_geometry_calls_with_goals_equal_pose_geometry_of_the_model_s_records(pt, renderer_mod, how):
    _ik_same_as_twin(pt, renderer_mod, m9_case(pt, renderer_mod, "linear"), how, ("skin", how))


def test_mix_pose_geometry_with_goals_under_the_dual_quaternion_rule(pt, renderer_mod):
    _ik_same_as_twin(pt, renderer_mod, m9_case(pt, renderer_mod, "dq", step=7), "mix", ("dq", "mix"))


def test_mix_pose_geometry_with_goals_under_the_part_rule(pt, renderer_mod):
    """M1 under the part rule (test_gpu_rig.m1_case's hierarchy: the sphere is the box's child): the sphere aims at a point, its first joint's
    parent the box"""
    case = m1_case(pt)
    case.update(clips={0: (case["times"], case["values"])}, masks={}, cons=[IM.aim(1, (0.0, 0.0, 1.0))], goals=[IM.goal((0.4, 0.1, -0.3), 0.37)])
    case["model"] = [MM.layer(0, 1.5)]
    case["layers"] = pack(renderer_mod, case["model"])
    _ik_same_as_twin(pt, renderer_mod, case, "mix", ("parts", "mix"))


def test_a_stale_pose_is_refused_under_each_call_s_name(pt, renderer_mod):
    case = m9_case(pt, renderer_mod, "linear")
    r = context(renderer_mod, case["old"], case["tex"], (case["rest"].W, case["rest"].H))
    frame(pt, r, 1)
    pose = case["make"](r)
    rig = make_rig(pose, case["parent"], case["bind"])
    rig.clip(case["times"], case["values"])
    fill(rig, case["clips"], case["masks"])
    attach(rig, case["cons"], case["goals"])
    assert rig.mix(case["layers"])[1] is True
    r.set_buffer(3, case["old"][3])
    for how, name in (("locals", "pt_rig_pose_geometry"), ("clip at a key", "pt_rig_clip_pose_geometry"), ("mix", "pt_rig_mix_pose_geometry")):
        with pytest.raises(renderer_mod.PtError) as e:
            _source(case, how)[0](rig)
        assert e.value.code == -4 and str(e.value).endswith(f"{name}: the scene was uploaded since pt_pose_create")
    src = _source(case, "mix")[1]
    same_floats(rig.mix_records(case["layers"]), IM.ik_records(case["parent"], case["cons"], case["goals"], src, case["bind"]), "the rule alone still answers")
    same_floats(rig.ik_locals(src), IM.ik_locals(case["parent"], case["cons"], case["goals"], src), "and the solve")
    r.close()
