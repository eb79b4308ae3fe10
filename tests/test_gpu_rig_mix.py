"""GPU: include/pt_rig_mix.h — pt_rig_mix_locals against the numpy model of the rule (tests/_rig_mix_model.py) bit for bit, pt_rig_mix_records
against pt_rig_records of those locals and against the rig's own clip, and pt_rig_mix_pose_geometry against a twin context on which
pt_pose_geometry ran with the downloaded records: every device record array byte for byte, the next frame, root_cost and in_place; the refusal
of a NaN key and what a later settle delivers; staleness, the multi-stream slow path, destroyed rigs and poses.  48 x 27 or 96 x 54, a frame or
two; the joint counts are the smallest at which the launch can go wrong: none, one, two, a wave and a lane, a block less one, a block, a block
and a lane, and 1000; one, two and eight layers over clips of one, two and four keys.

A NaN the rule generates equals any NaN: its sign and payload are the hardware's.  Everything else is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _move_cases as MC
import _rig_mix_model as MM
import _rig_model as RM
from test_gpu_move import context, frame, records, same_image, same_records
from test_gpu_pose import one_soup, same_floats
from test_gpu_rig import NAN_TEXT, _run, m1_case, make_rig

pytestmark = pytest.mark.gpu

f32 = np.float32


def pack(renderer_mod, layers):
    """the model's layers as the 24-byte records"""
    return renderer_mod.rig_layers([dict(clip=y["clip"], t=y["t"], weight=y["weight"], mask=y["mask"], mode=y["mode"], wrap=y["wrap"]) for y in layers])


def fill(rig, clips, masks):
    assert hasattr(rig._L, "pt_rig_mix_clip") and hasattr(rig, "mix_clip")      # never skipped: a library without the symbol fails here
    for slot, (times, values) in clips.items():
        rig.mix_clip(slot, times, values)
    for slot, w in masks.items():
        rig.mask(slot, w)


def tree(n):
    return RM.forest(n, 7) if n >= 65 else RM.chain(n)


@pytest.fixture(scope="module")
def bench(pt, renderer_mod):
    """a context over a soup of 4 triangles, all static: poses of any n_parts for the rule alone"""
    b = one_soup(pt, 4)
    r = context(renderer_mod, b, MC.SKY, (MC.W, MC.H))
    yield r, np.full(4, -1, np.int32)
    r.close()


# ------------------------------------------------------------------------------------------------ the rule alone

MIX_CASES = MM.mix_cases()


@pytest.mark.parametrize("k", range(len(MIX_CASES)), ids=["-".join(c[0]).replace(" ", "_") for c in MIX_CASES])
def test_mix_locals_equal_the_model_bit_for_bit(bench, renderer_mod, k):
    r, static = bench
    tag, n, clips, masks, layers = MIX_CASES[k]
    parent, bind = tree(n), RM.random_binds(n, 3)
    pose = r.pose_create(static, n)
    rig = make_rig(pose, parent, bind)
    fill(rig, clips, masks)
    y = pack(renderer_mod, layers)
    want = MM.mix_locals(clips, masks, layers, n)
    got = rig.mix_locals(y)
    same_floats(got, want, tag)
    assert (got[:, 3] == 0).all() and (got[:, 11] == 0).all()              # step 7
    rec = rig.mix_records(y)
    same_floats(rec, rig.records(got), (tag, "the records are pt_rig_records of the mixed locals"))
    same_floats(rec, RM.records(parent, want, bind), (tag, "the records"))
    if n:                                                                  # the timed launch writes the same locals, and a following call answers the same
        best = C.c_float(-1.0)
        assert r._L.pt_debug_rig_mix_time(rig._h, y.ctypes.data, y.nbytes, 2, C.byref(best)) == 0, r._L.pt_last_error()
        assert best.value >= 0.0
        same_floats(rig.mix_locals(y), want, (tag, "again"))
    other = [MM.layer(3, 1.25), MM.layer(0, 0.75, 0.5, 7, MM.ADDITIVE)]    # a second mix on the same rig: nothing is left over from the first
    same_floats(rig.mix_locals(pack(renderer_mod, other)), MM.mix_locals(clips, masks, other, n), (tag, "other layers"))
    same_floats(rig.mix_records(y), rec, (tag, "and back"))
    rig.close(); pose.close()


def test_one_layer_equals_the_rig_s_own_clip_bit_for_bit(bench, renderer_mod):
    r, static = bench
    n = 257
    clips, masks = MM.slots(n)
    parent, bind = tree(n), RM.random_binds(n, 3)
    pose = r.pose_create(static, n)
    rig = make_rig(pose, parent, bind)
    fill(rig, clips, masks)
    times, values = clips[0]
    rig.clip(times, values)                                                # pt_rig_clip_attach's single clip, beside the slots
    for t in list(times) + [0.5, 1.125, 3.999, -3.0, 4.5, np.inf, -np.inf]:
        same_floats(rig.mix_records(pack(renderer_mod, [MM.layer(0, t)])), rig.records_at(t), ("one layer", float(t)))
    rig.clip(*clips[3])                                                    # the rig's clip replaced: the slots stay as they are
    same_floats(rig.mix_records(pack(renderer_mod, [MM.layer(0, 1.125)])), RM.clip_records(parent, times, values, f32(1.125), bind), "slot 0 after rig.clip")
    same_floats(rig.records_at(0.5), RM.clip_records(parent, *clips[3], f32(0.5), bind), "the rig's clip after the mix")
    rig.close(); pose.close()


def test_a_replaced_slot_answers_with_the_second_attach(bench, renderer_mod):
    r, static = bench
    n = 65
    clips, masks = MM.slots(n)
    pose = r.pose_create(static, n)
    rig = make_rig(pose, tree(n))
    fill(rig, clips, masks)
    layers = MM.LAYER_SETS["eight"]
    y = pack(renderer_mod, layers)
    first = MM.mix_locals(clips, masks, layers, n)
    same_floats(rig.mix_locals(y), first, "before")
    clips2 = dict(clips)
    clips2[3] = (np.array([0.5, 1.0, 3.0], f32), np.stack([RM.random_locals(n, 80 + k, unnormalised=False) for k in range(3)]))      # another key count too
    masks2 = dict(masks)
    masks2[7] = MM.ramp(n)[::-1].copy()
    rig.mix_clip(3, *clips2[3]); rig.mask(7, masks2[7])
    second = MM.mix_locals(clips2, masks2, layers, n)
    same_floats(rig.mix_locals(y), second, "after")
    assert not np.array_equal(first, second)
    L = renderer_mod.lib()
    bad = np.array([0.0, 0.5, 0.5], f32)                                   # a refused attach leaves the slot as it was
    v = clips2[3][1].reshape(-1)
    assert L.pt_rig_mix_clip(rig._h, 3, 3, bad.ctypes.data, bad.nbytes, v.ctypes.data, v.nbytes) == -1
    assert L.pt_last_error().decode() == "pt_rig_mix_clip: times must be finite and strictly increasing"
    same_floats(rig.mix_locals(y), second, "after a refused attach")
    rig.close(); pose.close()


def test_two_rigs_on_one_pose_do_not_meet(bench, renderer_mod):
    r, static = bench
    n = 65
    pose = r.pose_create(static, n)
    a, b = make_rig(pose, RM.chain(n)), make_rig(pose, RM.star(n - 1))
    ca, ma = MM.slots(n, seed=0)
    cb, mb = MM.slots(n, seed=500)
    fill(a, ca, ma); fill(b, cb, mb)
    layers = MM.LAYER_SETS["eight"]
    y = pack(renderer_mod, layers)
    want_a, want_b = MM.mix_locals(ca, ma, layers, n), MM.mix_locals(cb, mb, layers, n)
    same_floats(a.mix_locals(y), want_a, "a"); same_floats(b.mix_locals(y), want_b, "b"); same_floats(a.mix_locals(y), want_a, "a again")
    assert not np.array_equal(want_a, want_b)
    a.close(); b.close(); pose.close()


def test_a_live_rig_refuses_bad_layers_in_the_header_s_order(bench, renderer_mod):
    r, static = bench
    pose = r.pose_create(static, 2)
    rig = make_rig(pose, RM.chain(2))
    clips, masks = MM.slots(2)
    rig.mix_clip(0, *clips[0]); rig.mask(7, masks[7])
    cases = [([MM.layer(3, 0.5)], "layer 0: a clip slot outside [0, 16) or empty"), ([MM.layer(0, 0.5), MM.layer(0, 0.5, 0.5, 1)], "layer 1: a mask outside [-1, 8) or empty"),
             ([MM.layer(0, 0.5), MM.layer(0, np.nan, 0.5, 7)], "layer 1: t is NaN"), ([MM.layer(0, 0.5), MM.layer(0, np.inf, 0.5, 7, MM.OVERRIDE, MM.LOOP)], "layer 1: an infinite t with LOOP"),
             ([MM.layer(0, 0.5), MM.layer(0, 0.5, 1.5)], "layer 1: a weight must be finite and in [0, 1]"), ([MM.layer(0, 0.5, 1.0, 7)], "layer 0 must be OVERRIDE with mask -1 and weight 1"),
             ([MM.layer(0, 0.5)] * 9, "layer_bytes must be 24 times a layer count of 1 to 8"), ([], "null layers")]
    for layers, text in cases:
        for call, name in ((rig.mix_locals, "pt_rig_mix_locals"), (rig.mix_records, "pt_rig_mix_records"), (rig.mix, "pt_rig_mix_pose_geometry")):
            with pytest.raises(renderer_mod.PtError) as e:
                call(pack(renderer_mod, layers))
            assert e.value.code == -1 and str(e.value).endswith(f"{name}: {text}"), (name, text, str(e.value))
    same_floats(rig.mix_locals(pack(renderer_mod, [MM.layer(0, 0.5)])), MM.mix_locals(clips, masks, [MM.layer(0, 0.5)], 2), "the rig still answers")
    rig.close(); pose.close()


# ------------------------------------------------------------------------------------------------ equivalence with pt_pose_geometry on a twin

def m8_case(pt, renderer_mod, blend, chained=False, step=3):
    """M8 (M7's chain with two clips in slots and a ramp mask) under the linear or the dual-quaternion skin; chained: M5's morph ahead and
    recomputed normals behind"""
    wl, bone, weight, parent, bind, clips, mask, layers = pt.scenes.m8_mixed(step)
    old, tex = MC.workload_inputs(wl)

    def make(r):
        pose = r.skin_create(bone, weight, 5, blend=blend)
        if chained:
            _, _, _, targets, _, w4, ids, nv = pt.scenes.m5_rippling(3)
            pose.morph_attach(targets); pose.normals_attach(ids, nv); pose.morph_weights(w4)
        return pose
    y = renderer_mod.rig_layers(layers)
    model = [MM.layer(int(a["clip"]), a["t"], a["weight"], int(a["mask"]), int(a["mode"]), int(a["wrap"])) for a in y]
    return dict(rest=wl, old=old, tex=tex, make=make, parent=parent, bind=bind, times=clips[0][0], values=clips[0][1], clips={0: clips[0], 1: clips[1]}, masks={0: mask},
                layers=y, model=model)


def _run_mix(pt, renderer_mod, case, layers, **opts):
    """test_gpu_rig._run's steps with the mix as the step: a frame, the step, the records at once, the next frame, the records after it"""
    r = context(renderer_mod, case["old"], case["tex"], (case["rest"].W, case["rest"].H), **opts)
    frame(pt, r, 1)
    pose = case["make"](r)
    rig = make_rig(pose, case["parent"], case["bind"])
    rig.clip(case["times"], case["values"])
    fill(rig, case["clips"], case["masks"])
    R = rig.mix_records(layers)
    cost, in_place = rig.mix(layers)
    out = (cost, in_place, records(r, skip=("ellip",)), frame(pt, r, 2), records(r), R)
    rig.close(); pose.close(); r.close()
    return out


def _mix_same_as_twin(pt, renderer_mod, case, tag, **opts):
    cost, flag, at_once, img, after, R = _run_mix(pt, renderer_mod, case, case["layers"], **opts)
    same_floats(R, MM.mix_records(case["parent"], case["clips"], case["masks"], case["model"], case["bind"]), (tag, "the records"))
    cost2, flag2, at_once2, img2, after2, _ = _run(pt, renderer_mod, case, "twin", R, **opts)      # pt_pose_geometry with the downloaded records
    assert flag is True and flag2 is True, (tag, flag, flag2)                # in_place, and equal
    assert np.array_equal(cost.view(np.uint64), cost2.view(np.uint64)) and cost.size == int(case["old"][13][0]), tag      # root_cost
    same_records(at_once, at_once2, (tag, "before the next render"))
    same_records(after, after2, tag)
    same_image(img, img2, tag)
    return after


@pytest.mark.parametrize("name", ["skin", "dq", "chained"])
def test_mix_pose_geometry_equals_pose_geometry_of_the_downloaded_records(pt, renderer_mod, name):
    blend = "dq" if name == "dq" else "linear"
    moved = _mix_same_as_twin(pt, renderer_mod, m8_case(pt, renderer_mod, blend, chained=name == "chained"), (name, "step 3"))
    if name == "skin":
        later = _mix_same_as_twin(pt, renderer_mod, m8_case(pt, renderer_mod, blend, step=7), (name, "step 7"))
        assert not np.array_equal(moved["tris"], later["tris"])               # a step is a function of its number


def test_mix_pose_geometry_under_the_part_rule(pt, renderer_mod):
    """M1 under the part rule (test_gpu_rig.m1_case's hierarchy): its clip in slot 0, a second clip in slot 5, the poster masked out"""
    case = m1_case(pt)
    v2 = case["values"].copy()
    v2[:, :, 0:3] = v2[:, :, 0:3] * f32(-0.5)
    case.update(clips={0: (case["times"], case["values"]), 5: (np.array([0.0, 3.0], f32), v2[[0, 2]])}, masks={2: np.array([1.0, 0.5, 0.0], f32)})
    case["model"] = [MM.layer(0, 1.5), MM.layer(5, 7.0, 0.75, 2, MM.OVERRIDE, MM.LOOP), MM.layer(0, 0.5, 0.5, -1, MM.ADDITIVE)]
    case["layers"] = pack(renderer_mod, case["model"])
    _mix_same_as_twin(pt, renderer_mod, case, ("parts", "three layers"))


# ------------------------------------------------------------------------------------------------ refusal and restore

def test_a_nan_key_is_refused_and_a_later_settle_delivers_the_last_accepted_pose(pt, renderer_mod):
    case = m8_case(pt, renderer_mod, "linear")
    L = renderer_mod.lib()
    bad = case["clips"][1][1].copy()
    bad[:, 3, 0] = np.nan                                                   # joint 3's translation in every key of the twist
    size = (case["rest"].W, case["rest"].H)
    r = context(renderer_mod, case["old"], case["tex"], size, asm_node_layout=0)
    frame(pt, r, 1)
    pose = case["make"](r)
    rig = make_rig(pose, case["parent"], case["bind"])
    fill(rig, case["clips"], case["masks"])
    rig.mix_clip(9, case["clips"][1][0], bad)
    good = case["layers"]
    poisoned = good.copy()
    poisoned["clip"][1] = 9
    assert np.isnan(rig.mix_records(poisoned)[3:, :12]).any()               # the rule alone hands the NaN on

    def refused():
        flag, cost = C.c_int(-5), np.full(pose.n_roots, -7.0)
        rc = L.pt_rig_mix_pose_geometry(r._h, rig._h, poisoned.ctypes.data, poisoned.nbytes, None, 0, cost.ctypes.data, C.byref(flag))
        assert rc == -4 and L.pt_last_error().decode() == f"pt_rig_mix_pose_geometry: {NAN_TEXT}"      # PT_ERR_SCENE, under this call's name
        assert flag.value == -5 and (cost == -7.0).all()

    img0, before0 = frame(pt, r, 2), records(r)
    refused()                                                               # no accepted pose yet: the rest pose stays
    same_records(records(r), before0, "refused first")
    same_image(frame(pt, r, 2), img0, "refused first")
    assert rig.mix(good)[1] is True                                         # the rig is still usable
    R = rig.mix_records(good)
    img, before = frame(pt, r, 2), records(r)
    refused()
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

def test_a_stale_pose_is_refused_under_the_mix_s_name(pt, renderer_mod):
    case = m8_case(pt, renderer_mod, "linear")
    r = context(renderer_mod, case["old"], case["tex"], (case["rest"].W, case["rest"].H))
    frame(pt, r, 1)
    pose = case["make"](r)
    rig = make_rig(pose, case["parent"], case["bind"])
    fill(rig, case["clips"], case["masks"])
    assert rig.mix(case["layers"])[1] is True
    r.set_buffer(3, case["old"][3])
    with pytest.raises(renderer_mod.PtError) as e:
        rig.mix(case["layers"])
    assert e.value.code == -4 and str(e.value).endswith("pt_rig_mix_pose_geometry: the scene was uploaded since pt_pose_create")
    same_floats(rig.mix_records(case["layers"]), MM.mix_records(case["parent"], case["clips"], case["masks"], case["model"], case["bind"]), "the rule alone still answers")
    r.close()


def test_a_rig_of_another_context_is_refused(pt, renderer_mod, bench):
    r, static = bench
    pose = r.pose_create(static, 2)
    rig = make_rig(pose, RM.chain(2))
    clips, masks = MM.slots(2)
    fill(rig, clips, masks)
    other = context(renderer_mod, one_soup(pt, 4), MC.SKY, (MC.W, MC.H))
    L = renderer_mod.lib()
    y = pack(renderer_mod, [MM.layer(0, 0.5)])
    assert L.pt_rig_mix_pose_geometry(other._h, rig._h, y.ctypes.data, y.nbytes, None, 0, None, None) == -1
    assert L.pt_last_error().decode() == "pt_rig_mix_pose_geometry: the rig's pose was created on another context"
    other.close(); rig.close(); pose.close()


def test_slow_path_multi_stream_context(pt, renderer_mod):
    case = m8_case(pt, renderer_mod, "linear")
    rest = case["rest"]
    r = renderer_mod.Renderer(rest.W, rest.H, devices=[0, 0])
    r.load_workload(rest)
    frame(pt, r, 1)
    pose = case["make"](r)
    rig = make_rig(pose, case["parent"], case["bind"])
    fill(rig, case["clips"], case["masks"])
    R = rig.mix_records(case["layers"])
    same_floats(R, MM.mix_records(case["parent"], case["clips"], case["masks"], case["model"], case["bind"]), "multi")
    cost, in_place = rig.mix(case["layers"])
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
    clips, masks = MM.slots(3)
    y = pack(renderer_mod, [MM.layer(0, 0.5)])
    x, w, loc, rec = clips[15][1].reshape(-1), masks[7], np.zeros(36, f32), np.zeros(72, f32)

    def refused(h):
        assert L.pt_rig_mix_locals(h, y.ctypes.data, y.nbytes, loc.ctypes.data, loc.nbytes) == -1 and L.pt_last_error().decode() == "pt_rig_mix_locals: null or destroyed rig"
        assert L.pt_rig_mix_records(h, y.ctypes.data, y.nbytes, rec.ctypes.data, rec.nbytes) == -1 and L.pt_last_error().decode() == "pt_rig_mix_records: null or destroyed rig"
        assert L.pt_rig_mix_pose_geometry(r._h, h, y.ctypes.data, y.nbytes, None, 0, None, None) == -1
        assert L.pt_last_error().decode() == "pt_rig_mix_pose_geometry: null or destroyed rig"
        assert L.pt_rig_mix_clip(h, 0, 1, x.ctypes.data, 4, x.ctypes.data, x.nbytes) == -1 and L.pt_last_error().decode() == "pt_rig_mix_clip: null or destroyed rig"
        assert L.pt_rig_mix_mask(h, 0, w.ctypes.data, w.nbytes) == -1 and L.pt_last_error().decode() == "pt_rig_mix_mask: null or destroyed rig"

    pose = r.pose_create(static, 3)
    rig, keep = make_rig(pose, RM.star(2)), make_rig(pose, RM.chain(3))
    fill(rig, clips, masks); fill(keep, clips, masks)
    h = C.c_void_p(rig._h.value)
    rig.close()                                                             # the slots go with their rig
    refused(h)
    same_floats(keep.mix_locals(y), MM.mix_locals(clips, masks, [MM.layer(0, 0.5)], 3), "the pose's other rig lives on")
    h = C.c_void_p(keep._h.value)
    pose.close()                                                            # pt_pose_destroy destroys the pose's rigs
    refused(h)
    keep._h = None
    ctx = context(renderer_mod, one_soup(pt, 4), MC.SKY, (MC.W, MC.H))     # pt_destroy destroys the poses' rigs
    p2 = ctx.pose_create(static, 3)
    g2 = make_rig(p2, RM.chain(3))
    fill(g2, clips, masks)
    h2 = C.c_void_p(g2._h.value)
    ctx.close()
    refused(h2)
    assert not loc.any() and not rec.any()
    g2._h = None; p2._h = None


# ------------------------------------------------------------------------------------------------ one rig, every source, any order

def test_one_rig_answers_locals_clip_and_mix_calls_in_any_order(bench, renderer_mod):
    """The caller's locals, the own clip and a mix share the rig's dLocals, and a time at a key reads the clip in place: seven calls of the three
    sources interleaved on one rig, each against its model bit for bit, then the same calls in reverse order, each the same bits as before.
    Five joints over three levels, one of them three joints wide; the mix has two layers over its base, one masked and one additive."""
    r, static = bench
    n = 5
    parent, bind = np.array([-1, 0, 1, 0, 0], np.int32), RM.random_binds(n, 3)
    pose = r.pose_create(static, n)
    rig = make_rig(pose, parent, bind)
    times, values = np.array([0.0, 1.0, 2.5], f32), np.stack([RM.random_locals(n, 40 + k) for k in range(3)])
    clips = {0: (np.array([0.5, 2.0], f32), np.stack([RM.random_locals(n, 50 + k) for k in range(2)])),
             1: (np.array([0.0, 1.0, 3.0], f32), np.stack([RM.random_locals(n, 55 + k, unnormalised=False) for k in range(3)]))}
    masks = {0: np.array([0.0, 1.0, 0.25, 0.5, 1.0], f32)}
    rig.clip(times, values)
    fill(rig, clips, masks)
    A, B = RM.random_locals(n, 60), RM.random_locals(n, 61)
    layers = [MM.layer(1, 1.5), MM.layer(0, 1.0, 0.75, 0), MM.layer(1, 0.5, 0.5, -1, MM.ADDITIVE)]
    y = pack(renderer_mod, layers)
    at = lambda t: RM.clip_records(parent, times, values, f32(t), bind)
    assert RM.interval(times, f32(1.0))[0] == 1 and RM.interval(times, f32(1.75))[0] < 0 and RM.interval(times, f32(0.0))[0] == 0
    calls = [("records(A)", lambda: rig.records(A), RM.records(parent, A, bind)),
             ("records_at(key 1)", lambda: rig.records_at(1.0), at(1.0)),
             ("mix_records", lambda: rig.mix_records(y), MM.mix_records(parent, clips, masks, layers, bind)),
             ("records_at(between keys 1 and 2)", lambda: rig.records_at(1.75), at(1.75)),
             ("records(B)", lambda: rig.records(B), RM.records(parent, B, bind)),
             ("mix_locals", lambda: rig.mix_locals(y), MM.mix_locals(clips, masks, layers, n)),
             ("records_at(key 0)", lambda: rig.records_at(0.0), at(0.0))]
    forward = []
    for tag, call, want in calls:
        forward.append(call())
        same_floats(forward[-1], want, tag)
    for (tag, call, _), was in reversed(list(zip(calls, forward))):
        assert np.array_equal(call().view(np.uint32), was.view(np.uint32)), (tag, "reversed")
    assert len({a.tobytes() for a in forward}) == len(forward)              # seven different answers: none is another call's left over
    times2, values2 = np.array([0.25, 1.0], f32), np.stack([RM.random_locals(n, 70), RM.random_locals(n, 71)])
    rig.clip(times2, values2)                                               # the own clip replaced, by one of another key count: the slots stay
    for t in (0.25, 0.5, 1.0, 2.5):
        same_floats(rig.records_at(t), RM.clip_records(parent, times2, values2, f32(t), bind), ("replaced", t))
    one = [MM.layer(1, 1.5)]
    same_floats(rig.mix_records(pack(renderer_mod, one)), MM.mix_records(parent, clips, masks, one, bind), "slot 1 after rig.clip")
    rig.close(); pose.close()
