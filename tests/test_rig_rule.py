"""CPU: the host-only step of include/pt_rig.h (csrc/hip/pt_rig_rule.hpp) through tests/c/rig_rule_check.cpp, a stand-alone program built twice
with g++: plain, and under the address / undefined-behaviour sanitizers (which must stay silent and agree).  Every refusal in the header's order;
the level plan against the model; the C++ statement of steps 1-5 against tests/_rig_model.py bit for bit on the cases the GPU test runs; the
model against the binary64 evaluation of tests/_rig_ref64.py within the bound derived there, and two mutations that the bound must notice.

A NaN the rule generates (0 / 0 under a zero scale) equals any NaN: its sign and payload are the hardware's.  Everything else, the infinities
included, is compared bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import _rig_model as RM
import _rig_ref64 as R64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NAN = "7fc00000"


def _words(a):
    return " ".join(f"{w:08x}" for w in np.ascontiguousarray(a, f32).reshape(-1).view(np.uint32))


def _word(x):
    return _words(np.array([x], f32))


# ------------------------------------------------------------------------------------------------ the refusals: fields in the header's order
# per call: (kind, the good request as a dict, [(field, bad value, RigCheck, text)] in the order the header lists the refusals)

RG = {name: k for k, name in enumerate("OK NULL POSE PARENT_BYTES PARENT BIND_BYTES DEPTH RIG FOREIGN LOCALS LOCAL_BYTES OUT RECORD_BYTES NO_CLIP NAN_T N_KEYS CLIP_NULL "
                                       "TIME_BYTES VALUE_BYTES TIMES ELLIP_BYTES".split())}
DEEP = list(range(-1, RM.MAX_DEPTH))                                   # 257 joints in one chain: depth 257
CALLS = {
    "pt_rig_create": ("K", dict(pose=1, live=1, parent=1, out=1, parent_bytes=12, bind=1, bind_bytes=144, n_parts=3, parents=[-1, 0, 0]), [
        ("pose", 0, "NULL", "null pose, parent or out"), ("live", 0, "POSE", "the pose is not live"), ("parent_bytes", 16, "PARENT_BYTES", "parent_bytes != n_parts * 4"),
        ("parents", [-1, 1, 0], "PARENT", "a parent outside [-1, j)"), ("bind_bytes", 140, "BIND_BYTES", "bind_bytes != n_parts * 48"),
        ("deep", 1, "DEPTH", "a depth above PT_RIG_MAX_DEPTH (256)")]),
    "pt_rig_records": ("R", dict(live=1, locals=1, local_bytes=144, out=1, record_bytes=288, n_parts=3), [
        ("live", 0, "RIG", "null or destroyed rig"), ("locals", 0, "LOCALS", "null locals with n_parts > 0"), ("local_bytes", 143, "LOCAL_BYTES", "local_bytes != n_parts * 48"),
        ("out", 0, "OUT", "null records_out"), ("record_bytes", 144, "RECORD_BYTES", "record_bytes != n_parts * 96")]),
    "pt_rig_clip_records": ("T", dict(live=1, clip=1, t="3f000000", out=1, record_bytes=288, n_parts=3), [
        ("live", 0, "RIG", "null or destroyed rig"), ("clip", 0, "NO_CLIP", "no clip attached"), ("t", NAN, "NAN_T", "t is NaN"), ("out", 0, "OUT", "null records_out"),
        ("record_bytes", 0, "RECORD_BYTES", "record_bytes != n_parts * 96")]),
    "pt_rig_clip_attach": ("A", dict(live=1, n_keys=2, times=1, time_bytes=8, values=1, value_bytes=288, n_parts=3, ts=[0.0, 1.0]), [
        ("live", 0, "RIG", "null or destroyed rig"), ("n_keys", 0, "N_KEYS", "n_keys < 1"), ("values", 0, "CLIP_NULL", "null times, or null values with n_parts > 0"),
        ("time_bytes", 12, "TIME_BYTES", "time_bytes != n_keys * 4"), ("value_bytes", 144, "VALUE_BYTES", "value_bytes != n_keys * n_parts * 48"),
        ("ts", [1.0, 1.0], "TIMES", "times must be finite and strictly increasing")]),
    "pt_rig_pose_geometry": ("G", dict(clip_call=0, ctx=1, live=1, own=1, locals=1, local_bytes=144, clip=0, t=NAN, n_parts=3, ellip=1, ellip_bytes=64), [
        ("ctx", 0, "NULL", "null ctx"), ("live", 0, "RIG", "null or destroyed rig"), ("own", 0, "FOREIGN", "the rig's pose was created on another context"),
        ("locals", 0, "LOCALS", "null locals with n_parts > 0"), ("local_bytes", 96, "LOCAL_BYTES", "local_bytes != n_parts * 48"),
        ("ellip_bytes", 62, "ELLIP_BYTES", "ellip_bytes must be a multiple of 4 bytes")]),
    "pt_rig_clip_pose_geometry": ("G", dict(clip_call=1, ctx=1, live=1, own=1, locals=0, local_bytes=7, clip=1, t="3f800000", n_parts=3, ellip=1, ellip_bytes=64), [
        ("ctx", 0, "NULL", "null ctx"), ("live", 0, "RIG", "null or destroyed rig"), ("own", 0, "FOREIGN", "the rig's pose was created on another context"),
        ("clip", 0, "NO_CLIP", "no clip attached"), ("t", NAN, "NAN_T", "t is NaN"), ("ellip_bytes", 62, "ELLIP_BYTES", "ellip_bytes must be a multiple of 4 bytes")]),
}


def _line(kind, r):
    if kind == "K":
        deep = bool(r.get("deep"))                                     # the chain of 257 joints, its byte counts right where the request's were
        parents = DEEP if deep else r["parents"]
        n = len(parents) if deep else r["n_parts"]
        pb = 4 * n if deep and r["parent_bytes"] == 12 else r["parent_bytes"]
        bb = 48 * n if deep and r["bind_bytes"] == 144 else r["bind_bytes"]
        return f"K {r['pose']} {r['live']} {r['parent']} {r['out']} {pb} {r['bind']} {bb} {n} " + " ".join(str(p) for p in parents[:n])
    if kind == "R":
        return f"R {r['live']} {r['locals']} {r['local_bytes']} {r['out']} {r['record_bytes']} {r['n_parts']}"
    if kind == "T":
        return f"T {r['live']} {r['clip']} {r['t']} {r['out']} {r['record_bytes']} {r['n_parts']}"
    if kind == "A":
        ts = r["ts"][:max(r["n_keys"], 0)]
        return f"A {r['live']} {r['n_keys']} {r['times']} {r['time_bytes']} {r['values']} {r['value_bytes']} {r['n_parts']} " + _words(ts)
    return (f"G {r['clip_call']} {r['ctx']} {r['live']} {r['own']} {r['locals']} {r['local_bytes']} {r['clip']} {r['t']} {r['n_parts']} {r['ellip']} "
            f"{r['ellip_bytes']}")


def check_requests():
    """(lines, expectations): per call the good request, each fault alone, and each ordered pair of faults (the earlier field answers)"""
    lines, want = [], []
    for who, (kind, good, faults) in CALLS.items():
        lines.append(_line(kind, good)); want.append((who, None))
        for i, (field, value, check, text) in enumerate(faults):
            lines.append(_line(kind, dict(good, **{field: value}))); want.append((who, (check, text)))
            for field2, value2, _, _ in faults[i + 1:]:
                if "deep" in (field, field2) and "parents" in (field, field2):
                    continue                                           # (one table of parents per request)
                lines.append(_line(kind, dict(good, **{field: value, field2: value2}))); want.append((who, (check, text)))
    # the other null arguments of pt_rig_create, the other faults of a clip's times, what n_parts == 0 allows
    extra = [("K", dict(CALLS["pt_rig_create"][1], parent=0), "pt_rig_create", ("NULL", "null pose, parent or out")),
             ("K", dict(CALLS["pt_rig_create"][1], out=0), "pt_rig_create", ("NULL", "null pose, parent or out")),
             ("K", dict(CALLS["pt_rig_create"][1], parents=[-2, 0, 0]), "pt_rig_create", ("PARENT", "a parent outside [-1, j)")),
             ("K", dict(CALLS["pt_rig_create"][1], parents=[0, 0, 0]), "pt_rig_create", ("PARENT", "a parent outside [-1, j)")),
             ("K", dict(CALLS["pt_rig_create"][1], bind=0, bind_bytes=5), "pt_rig_create", None),                      # no inv_bind: its byte count is not read
             ("K", dict(pose=1, live=1, parent=1, out=1, parent_bytes=0, bind=0, bind_bytes=0, n_parts=0, parents=[]), "pt_rig_create", None),
             ("K", dict(pose=1, live=1, parent=1, out=1, parent_bytes=4 * 256, bind=0, bind_bytes=0, n_parts=256, parents=DEEP[:256]), "pt_rig_create", None),
             ("A", dict(CALLS["pt_rig_clip_attach"][1], times=0), "pt_rig_clip_attach", ("CLIP_NULL", "null times, or null values with n_parts > 0")),
             ("A", dict(CALLS["pt_rig_clip_attach"][1], ts=[1.0, 0.5]), "pt_rig_clip_attach", ("TIMES", "times must be finite and strictly increasing")),
             ("A", dict(CALLS["pt_rig_clip_attach"][1], ts=[0.0, np.inf]), "pt_rig_clip_attach", ("TIMES", "times must be finite and strictly increasing")),
             ("A", dict(CALLS["pt_rig_clip_attach"][1], ts=[np.nan, 1.0]), "pt_rig_clip_attach", ("TIMES", "times must be finite and strictly increasing")),
             ("A", dict(CALLS["pt_rig_clip_attach"][1], n_keys=-1), "pt_rig_clip_attach", ("N_KEYS", "n_keys < 1")),
             ("A", dict(live=1, n_keys=1, times=1, time_bytes=4, values=0, value_bytes=0, n_parts=0, ts=[2.0]), "pt_rig_clip_attach", None),
             ("R", dict(live=1, locals=0, local_bytes=0, out=1, record_bytes=0, n_parts=0), "pt_rig_records", None),
             ("R", dict(live=1, locals=0, local_bytes=0, out=0, record_bytes=0, n_parts=0), "pt_rig_records", ("OUT", "null records_out")),
             ("T", dict(CALLS["pt_rig_clip_records"][1], t="7f800000"), "pt_rig_clip_records", None),                   # an infinite t is clamped, not refused
             ("G", dict(CALLS["pt_rig_pose_geometry"][1], ellip=0, ellip_bytes=3), "pt_rig_pose_geometry", None)]      # no ellipsoids: their byte count is not read
    for kind, r, who, w in extra:
        lines.append(_line(kind, r)); want.append((who, w))
    return lines, want


# ------------------------------------------------------------------------------------------------ the rule's cases

def rule_cases():
    """(tag, parent, locals, inv_bind or None): the hierarchies of the GPU test, inv_bind NULL and given, unnormalised q, a zero scale"""
    out = []
    for tag, parent in RM.hierarchies():
        n = parent.size
        l = RM.case_locals(tag, n)
        out.append(((tag, "plain"), parent, l, None))
        out.append(((tag, "bind"), parent, l, RM.random_binds(n, 3)))
        if n >= 2:
            out.append(((tag, "zero scale"), parent, RM.with_zero_scale(l), RM.random_binds(n, 4) if n % 2 else None))
    return out


def clip_cases():
    """(tag, parent, inv_bind, times, values, t): t at every key, between keys, before and after the clip, one key, keys q and -q"""
    out = []
    parent = RM.forest(40, 3, roots_at_end=2)
    times = np.array([0.25, 1.0, 1.5, 4.0], f32)
    values = np.stack([RM.random_locals(40, 20 + k) for k in range(4)])
    values[2, :, 4:8] = -values[1, :, 4:8] * f32(1.25)                   # keys 1 and 2: q and a multiple of -q
    bind = RM.random_binds(40, 9)
    for t in list(times) + [0.5, 1.125, 1.25, 3.999, np.nextafter(f32(1.0), f32(0)), -3.0, 0.0, 4.5, np.inf, -np.inf]:
        out.append((("forest40", float(t)), parent, bind, times, values, f32(t)))
    for t in (-1.0, 0.0, 7.0):
        out.append((("one key", t), parent, None, times[:1], values[:1], f32(t)))
    out.append((("none", 0.5), np.zeros(0, np.int32), None, times[:2], np.zeros((2, 0, 12), f32), f32(0.5)))
    return out


def _build(tmp, name, extra):
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "c", "rig_rule_check.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr      # no warning either
    return exe


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    assert os.path.exists(os.path.join(ROOT, "pathtracer-0_amd", "csrc", "hip", "pt_rig_rule.hpp"))
    tmp = tmp_path_factory.mktemp("rig_rule")
    path = str(tmp / "requests.txt")
    (lines, want), rules, clips = check_requests(), rule_cases(), clip_cases()
    plans = [p for _, p in RM.hierarchies()] + [RM.forest(200, 5), RM.star(3)]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
        for p in plans:
            f.write(f"P {p.size} " + " ".join(str(int(x)) for x in p) + "\n")
        for tag, parent, l, bind in rules:
            f.write(f"E {parent.size} {int(bind is not None)} " + " ".join(str(int(x)) for x in parent) + " " + _words(l) + (" " + _words(bind) if bind is not None else "") + "\n")
        for tag, parent, bind, times, values, t in clips:
            f.write(f"C {parent.size} {int(bind is not None)} {times.size} {_word(t)} " + " ".join(str(int(x)) for x in parent) + " " + _words(times) + " " + _words(values)
                    + (" " + _words(bind) if bind is not None else "") + "\n")
    got = []
    for exe in (_build(tmp, "check_plain", []), _build(tmp, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0 and run.stderr == "", (exe, run.returncode, run.stderr[-2000:])
        got.append(run.stdout.splitlines())
    assert got[0] == got[1] and len(got[0]) == len(lines) + len(plans) + len(rules) + len(clips)
    a, b, c = len(lines), len(lines) + len(plans), len(lines) + len(plans) + len(rules)
    return dict(checks=(lines, want, got[0][:a]), plans=(plans, got[0][a:b]), rules=(rules, got[0][b:c]), clips=(clips, got[0][c:]))


def test_every_refusal_in_the_header_s_order(answers):
    lines, want, got = answers["checks"]
    seen = set()
    for line, (who, w), g in zip(lines, want, got):
        code, which, text = (g.split(" ", 2) + [""])[:3]
        if w is None:
            assert (int(code), int(which), text) == (0, 0, ""), (line, g)
        else:
            assert int(code) == -1 and int(which) == RG[w[0]] and text == f"{who}: {w[1]}", (line, g)      # PT_ERR_ARG, under the entry point's name
            seen.add((who, w[0]))
    for who, (_, _, faults) in CALLS.items():
        assert {(who, c) for _, _, c, _ in faults} <= seen                # every listed refusal is reached
    assert {c for _, c in seen} == set(RG) - {"OK"}


def test_the_level_plan_equals_the_model_s(answers):
    plans, got = answers["plans"]
    widths = set()
    for parent, line in zip(plans, got):
        w = [int(x) for x in line.split()]
        order, start = RM.level_plan(parent)
        n = parent.size
        assert w[0] == len(start) - 1 and w[1:1 + n] == order.tolist() and w[1 + n:] == start.tolist(), parent[:10]
        d = RM.depths(parent)
        for l in range(len(start) - 1):                                   # a level's joints have its depth, ascend, and their parents lie one level up
            js = order[start[l]:start[l + 1]]
            assert (d[js] == l + 1).all() and (np.diff(js) > 0).all() and (l == 0 or (d[parent[js]] == l).all())
            widths.add(len(js))
    assert {1, 300} <= widths and any(w > 1 and w % 64 for w in widths)
    assert RM.depths(RM.chain(RM.MAX_DEPTH)).max() == RM.MAX_DEPTH


def _records_of(line, n, skip=0):
    w = line.split()[skip:]
    words = np.array([int(x, 16) for x in w], np.uint32).view(f32)
    return words[:24 * n].reshape(n, 24), words[24 * n:]


def test_the_cpp_rule_equals_the_model_bit_for_bit(answers):
    rules, got = answers["rules"]
    seen_inf = seen_nan = False
    for (tag, parent, l, bind), line in zip(rules, got):
        n = parent.size
        rec, world = _records_of(line, n, skip=1)
        want = RM.records(parent, l, bind)
        ok, bad = RM.same_floats(rec, want)
        assert ok, (tag, bad)
        ok, bad = RM.same_floats(world, RM.world(parent, l))
        assert ok, (tag, bad)
        assert (rec[:, 21:] == 0).all()
        roots = np.asarray(parent) < 0
        if n:
            assert np.array_equal(world.reshape(n, 12)[roots].view(np.uint32), RM.local_matrices(l)[roots].reshape(-1, 12).view(np.uint32))      # a root's W is its L
        if bind is None and n:
            assert np.array_equal(rec[:, :12].view(np.uint32), world.reshape(n, 12).view(np.uint32))                                          # M is W, bit for bit
        if tag[1] == "zero scale":
            seen_inf = seen_inf or bool(np.isinf(rec[:, 12:21]).any())
            seen_nan = seen_nan or bool(np.isnan(rec[:, 12:21]).any())
            assert np.isfinite(rec[:, :12]).all()
        else:
            assert np.isfinite(rec).all(), tag
    assert seen_inf and seen_nan
    assert {t[0] for t, *_ in rules} == {"one", "two", "chain65", "star300", "forest1000", "depth256", "none"}


def test_the_cpp_clip_equals_the_model_bit_for_bit(answers):
    clips, got = answers["clips"]
    exacts, flipped = set(), False
    for (tag, parent, bind, times, values, t), line in zip(clips, got):
        n = parent.size
        w = line.split()
        exact, k, u = RM.interval(times, t)
        assert (int(w[0]), int(w[1]), w[2]) == (exact, k, _word(u)), (tag, w[:3])
        rec, _ = _records_of(line, n, skip=3)
        ok, bad = RM.same_floats(rec, RM.clip_records(parent, times, values, t, bind))
        assert ok, (tag, bad)
        if exact >= 0:                                                    # at a key, and clamped: that key's own records, bit for bit
            ok, bad = RM.same_floats(rec, RM.records(parent, values[exact], bind))
            assert ok, (tag, bad)
            exacts.add((tag[0], exact))
        elif n:
            V = values.reshape(times.size, n, 12)
            flipped = flipped or bool(RM.flips(V[k], V[k + 1]).all())
            assert 0 < u < 1
    assert {("forest40", k) for k in range(4)} | {("one key", 0)} <= exacts and flipped


def test_keys_q_and_minus_q_blend_along_the_shorter_arc():
    """keys 1 and 2 of the clip hold q and -1.25 q: the same rotation.  Every blend between them is that rotation (the flip makes the lerp run
    from q to 1.25 q, not through zero), to the rounding of the normalisation"""
    _, parent, bind, times, values, _ = clip_cases()[0]
    a = RM.local_matrices(values[1])[:, :, :3]
    for t in (1.125, 1.25, 1.4):
        l = RM.clip_locals(times, values, parent.size, f32(t))
        R = RM.local_matrices(np.concatenate([values[1][:, :4], l[:, 4:8], values[1][:, 8:]], axis=1))[:, :, :3]
        # the blend's components carry E_q <= 3u (|v a| + |u b|) <= 3.75u |a| and the blend is at least as long as a: e_q = 3 * 3.75u + 4u,
        # e_R = 6 e_q + 5u = 96.5u; the key's own R carries 29u; both are scaled by s <= 1.5 and rounded once more: (125.5u + 2u) * 1.5 < 192u
        assert np.abs(R - a).max() < 192 * R64.U


# ------------------------------------------------------------------------------------------------ the binary64 reference and the derived bound

def _against_ref(tag, parent, l, bind, mutate=None):
    got = RM.records(parent, l, bind).astype(np.float64)
    ref, bound = R64.records(parent, l, bind, mutate=mutate)
    return got, ref, bound


def test_the_model_lies_within_the_derived_bound_of_the_binary64_evaluation():
    checked = 0
    for tag, parent, l, bind in rule_cases():
        if tag[1] == "zero scale" or parent.size == 0:
            continue
        got, ref, bound = _against_ref(tag, parent, l, bind)
        has = np.isfinite(bound)
        err = np.abs(got - ref)
        pos = has & (bound > 0)
        print(tag, "largest error", err[has].max(), "largest bound", bound[has].max(), "largest error / bound", (err[pos] / bound[pos]).max())
        assert has.mean() >= 0.99, tag                                    # these matrices are far from singular
        assert (err[has] <= bound[has]).all(), (tag, int((err[has] > bound[has]).sum()))
        assert (got[:, 21:] == 0).all() and (bound[:, 21:] == 0).all()
        checked += 1                                                      # (that the bound says something is test_the_bound_notices_a_mutation's to show)
    assert checked >= 12


@pytest.mark.parametrize("mutate", ["side", "transpose"])
def test_the_bound_notices_a_mutation(mutate):
    """the child composed on the wrong side, and N without its transpose: the binary32 model lies outside the bound of either"""
    for tag, parent, l, bind in rule_cases():
        if tag[0] not in ("chain65", "forest1000", "star300") or tag[1] != "bind":
            continue
        got, ref, bound = _against_ref(tag, parent, l, bind, mutate=mutate)
        has = np.isfinite(bound)
        outside = (np.abs(got - ref) > bound) & has
        cols = slice(12, 21) if mutate == "transpose" else slice(0, 12)
        assert outside[:, cols].any(axis=1).mean() > 0.9, (tag, mutate, outside[:, cols].any(axis=1).mean())
        if mutate == "transpose":
            assert not outside[:, :12].any()                              # M is untouched by this mutation


def test_a_clip_s_blend_lies_within_the_bound_too():
    for (tag, parent, bind, times, values, t) in clip_cases():
        exact, k, u = RM.interval(times, t)
        if exact >= 0 or parent.size == 0:
            continue
        V = values.reshape(times.size, parent.size, 12)
        if RM.flips(V[k], V[k + 1]).all():
            continue                                                      # q and -1.25 q: covered above
        l64, E = R64.blend(V[k], V[k + 1], u, RM.flips(V[k], V[k + 1]))
        short = np.linalg.norm(l64[:, 4:8], axis=1) < 0.25 * np.minimum(np.linalg.norm(V[k][:, 4:8], axis=1), np.linalg.norm(V[k + 1][:, 4:8], axis=1))
        assert not short.any()                                            # the shorter arc never passes near zero
        got = RM.clip_records(parent, times, values, t, bind).astype(np.float64)
        ref, bound = R64.records(parent, l64, bind, e_loc=E)
        has = np.isfinite(bound)
        err = np.abs(got - ref)
        print(tag, "largest error", err[has].max(), "largest bound", bound[has].max())
        assert has.mean() > 0.99 and (err[has] <= bound[has]).all(), (tag, int((err[has] > bound[has]).sum()))
