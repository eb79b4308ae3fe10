"""CPU: the argument table of the image-space calls (csrc/hip/pt_image_args.hpp) and the motion packing (csrc/hip/pt_motion_pack.hpp) through
tests/c/image_args_check.cpp, a stand-alone program that runs scripts of calls and prints what each answered.  Built twice with g++: plain, and
under the address / undefined-behaviour sanitizers (which must stay silent on every script, and agree).

  * every answer equals what the same arguments got before the table replaced the checks scattered over pt_hip.hip and pt_image.hpp
    (tests/golden/image_args_parent.json, recorded from that commit's own lines: see its "recorded" entry).  The scripts are generated here from
    the rows the program prints: per entry point an accepted base call, then one field at a time over a grid around every bound of the row (and
    every pointer absent), then every ordered pair of its fields and pointers both refused, which must answer as the earlier check does;
  * every row and every refusal text of the table is reached, every field is accepted at each of its bounds, and the rows are the functions
    the image-space headers declare plus pt_render_adaptive;
  * a build with one bound changed (iterations accepted up to 9) is seen by the golden;
  * the packed motion records equal the parent's bit for bit: flags 0, 1 and 2, a primitive beyond the mark's count, a NaN coordinate, a rot of
    -0.0, an ellipsoid buffer shorter than its count says, no primitive at all."""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from test_adaptive_abi import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "image_args_parent.json")
IMAGE_HEADERS = ("pt_denoise.h", "pt_guided.h", "pt_reproject.h", "pt_steer.h", "pt_demod.h", "pt_fill.h", "pt_through.h", "pt_motion.h", "pt_validate.h",
                 "pt_reproject_through.h", "pt_reproject_bilinear.h")
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
INF = float("inf")

# an accepted value of every field: the base call of every entry point is these (thru follows chains, so it has PT_THROUGH_KEY)
BASE = {"iterations": 3, "sigma0": 0.5, "sigma1": 1.0, "sigma2": 2.0, "sigma3": 4.0, "min_frames": 4, "albedo_floor": 0.01,
        "thru.max_depth": 2, "thru.min_weight": 0.25, "thru.lobes": 3, "thru.flags": 1,
        "guided.iterations": 2, "guided.sigma_lum": 1.5, "guided.sigma_normal": 0.25, "guided.sigma_depth": 0.125, "guided.sigma_albedo": 8.0, "guided.min_frames": 3,
        "guided.rel_err": 0.05, "guided.abs_err": 0.001, "guided.max_frames": 16,
        "validate.radius": 2, "validate.z_lo": 1.0, "validate.z_hi": 3.0, "validate.normal_tol": 0.9,
        "max_history": 64.0, "depth_tol": 0.05, "normal_tol": 0.8, "flags": 0, "point_tol": 0.02, "radius": 2, "snap": 0.25,
        "n_frames": 3, "stride": 4, "phase_x": 0, "phase_y": 0, "rel_err": 0.02, "abs_err": 0.002, "max_frames": 8}


def f32(x):
    return float(np.float32(x))


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def from_bits(u):
    return struct.unpack("<f", struct.pack("<I", u))[0]


def word(field, value):
    """field=value as the program reads it: ints in decimal, floats as the hex of their bits"""
    return f"{field}={value}" if isinstance(BASE[field], int) else f"{field}=f:{bits(value):08x}"


def key(value):
    """a value as a key of the golden file"""
    return str(value) if isinstance(value, int) else f"{bits(value):08x}"


# ------------------------------------------------------------------------------------------ the rows
def parse_table(lines):
    """the `table` command's lines -> [dict(name, prefix, checks=[dict(pred, own, fields, has, mask, ilo, ihi, lo, hi, lo_open, hi_open, text)])]"""
    rows = []
    for line in lines:
        if line.startswith("row "):
            _, name, prefix = line.split()
            rows.append(dict(name=name, prefix=prefix, checks=[]))
            continue
        head, text = line.split(" text=", 1)
        w = head.split()
        assert w[0] == "check"
        f = dict(kv.split("=", 1) for kv in w[2:])
        rows[-1]["checks"].append(dict(pred=w[1], own=f["own"] == "1", fields=[] if f["fields"] == "-" else f["fields"].split(","),
                                       has=[] if f["has"] == "-" else f["has"].split(","), mask=int(f["mask"]), ilo=int(f["ilo"]), ihi=int(f["ihi"]),
                                       lo=from_bits(int(f["lo"], 16)), hi=from_bits(int(f["hi"], 16)), lo_open=f["open"][0] == "1", hi_open=f["open"][1] == "1",
                                       text=text))
    return rows


def message(row, check):
    return (row["name"] if check["own"] else row["prefix"]) + ": " + check["text"]


def bounds_of(check):
    """{field: [(bound, the nearest value the check accepts at it)]} of one check, with the base values where a bound is another field"""
    def inside(b, is_open, up):
        return b if not is_open else f32(np.nextafter(np.float32(b), np.float32(INF if up else -INF)))
    p, fs = check["pred"], check["fields"]
    if p == "int_range":
        return {fs[0]: [(check["ilo"], check["ilo"]), (check["ihi"], check["ihi"])]}
    if p == "flags":
        return {fs[0]: [(0, 0), (check["mask"], check["mask"])]}
    if p == "interval":
        return {f: [(check["lo"], inside(check["lo"], check["lo_open"], True)), (check["hi"], inside(check["hi"], check["hi_open"], False))] for f in fs}
    if p == "phase":                                                  # [0, stride)
        return {f: [(0, 0), (BASE["stride"], BASE["stride"] - 1)] for f in fs[:2]}
    if p == "ordered":                                                # finite, 0 <= lo < hi
        lo, hi = fs
        return {lo: [(0.0, 0.0), (BASE[hi], inside(BASE[hi], True, False))], hi: [(BASE[lo], inside(BASE[lo], True, True)), (INF, inside(INF, True, False))]}
    return {}                                                         # present, keyed: no bound


def grid_of(field, bounds):
    """the values one field takes: every bound and its two neighbours, and the values every field of its type takes"""
    if isinstance(BASE[field], int):
        values = {0, -1, INT_MIN, INT_MAX}
        for b in bounds:
            values.update(v for v in (b - 1, b, b + 1) if INT_MIN <= v <= INT_MAX)
        return sorted(values)
    values = {bits(v) for v in (-0.0, from_bits(1), INF, -INF, float("nan"))}
    for b in bounds:
        values.update(bits(f32(v)) for v in (b, np.nextafter(np.float32(b), np.float32(-INF)), np.nextafter(np.float32(b), np.float32(INF))))
    return [from_bits(u) for u in sorted(values)]


def items_of(row):
    """(the row's pointers, its fields, {field: bounds}) in the order its checks name them"""
    pointers, fields, bounds = [], [], {}
    for check in row["checks"]:
        pointers += [p for p in check["has"] if p not in pointers]
        fields += [f for f in check["fields"] if f not in fields]
        for f, bs in bounds_of(check).items():
            bounds.setdefault(f, []).extend(b for b, _ in bs)
    return pointers, fields, bounds


def call_line(row, pointers, fields, change=()):
    """the base call of the row with `change` = ((item, value), ...): a pointer's value is False (absent), a field's its value"""
    change = dict(change)
    has = [p for p in pointers if change.get(p, True)]
    return " ".join([f"call {row['name']}", "has=" + (",".join(has) or "-")] + [word(f, change.get(f, BASE[f])) for f in fields])


def scripts_of(rows):
    """{entry point: {"base": line, "one": {item: {value key: line}}, "at_bounds": line}}; the pairs need the answers of these first (pairs_of)"""
    out = {}
    for row in rows:
        pointers, fields, bounds = items_of(row)
        one = {p: {"absent": call_line(row, pointers, fields, [(p, False)])} for p in pointers}
        for f in fields:
            one[f] = {key(v): call_line(row, pointers, fields, [(f, v)]) for v in grid_of(f, bounds.get(f, []))}
        lowest = {}                                                   # every field at the lower bound of the first check that bounds it
        for check in row["checks"]:
            for f, bs in bounds_of(check).items():
                lowest.setdefault(f, bs[0][1])
        assert set(lowest) == set(fields), row["name"]
        out[row["name"]] = dict(base=call_line(row, pointers, fields), one=one, at_bounds=call_line(row, pointers, fields, lowest.items()))
    return out


def pairs_of(rows, scripts, one):
    """{entry point: {"x|vx|y|vy": line}}: for every ordered pair of the row's items, x at its first refused value and y at its last"""
    out = {}
    for row in rows:
        pointers, fields, _ = items_of(row)
        name = row["name"]
        refused = {item: [v for v, answer in one[name][item].items() if not answer.startswith("rc=0 ")] for item in scripts[name]["one"]}

        def value(item, k):
            return False if item in pointers else int(k) if isinstance(BASE[item], int) else from_bits(int(k, 16))
        out[name] = {}
        for x in refused:
            for y in refused:
                if x != y and refused[x] and refused[y]:
                    vx, vy = refused[x][0], refused[y][-1]
                    out[name][f"{x}|{vx}|{y}|{vy}"] = call_line(row, pointers, fields, [(x, value(x, vx)), (y, value(y, vy))])
    return out


PACK_ONE = 0x3f800000


def _floats(values):
    return " ".join(f"{bits(f32(v)):08x}" for v in values)


def _binding7(ellipsoids, count=None):
    """[(centre, stretch, rot, r)] -> binding 7: the count, then the centres, the stretches, the rots, the radii, the materials"""
    n = len(ellipsoids)
    out = [float(n if count is None else count)]
    for k in range(3):
        out += [v for e in ellipsoids for v in e[k]]
    return out + [e[3] for e in ellipsoids] + [0.0] * n


def pack_scripts():
    nan = float("nan")
    t0, t1, t2 = [0, 0, 0, 1, 0, 0, 0, 1, 0], [1, 2, 3, 4, 5, 6, 7, 8, 9], [-1, -2, -3, 0.5, 0.25, 0.125, 9, 8, 7]
    still = ((1, 2, 3), (1, 1, 2), (0, 0, 0), 0.5)
    rotated = ((4, 5, 6), (2, 1, 1), (0.5, 0, 0), 0.75)

    def line(mode, *lists):
        return f"pack {mode} : " + " ; ".join(_floats(x) for x in lists)
    return {
        "nothing_mark": [line("mark", [], [])],
        "nothing_then": [line("then", [], [], [], [])],
        "mark": [line("mark", t0 + t1 + t2, _binding7([still, rotated]))],
        "unmoved": [line("then", t0 + t1, _binding7([still, rotated]), t0 + t1, _binding7([still, rotated]))],
        # flags 0, 1, 1 of the triangles; 0, 1 (no rot then or now), 2 (a rot now), 2 (a rot then) of the ellipsoids
        "flags": [line("then", t0 + [1, 2, 3, 4, 5, 6, 7, 8, 9.5] + [-1, -2, -3, 0.5, 0.25, 0.125, 9, 8, 7.5],
                       _binding7([still, ((1, 2, 3.5), (1, 1, 2), (0, 0, 0), 0.5), ((4, 5, 6), (2, 1, 1), (0.5, 0, 0), 0.8), ((4, 5, 6.5), (2, 1, 1), (0, 0, 0), 0.75)]),
                       t0 + t1 + t2, _binding7([still, still, rotated, rotated]))],
        "beyond_the_mark": [line("then", t0 + t1 + t2, _binding7([still, rotated, rotated]), t0, _binding7([still])),
                            line("then", t0, _binding7([still]), t0 + t1 + t2, _binding7([still, rotated]))],
        "nan_counts_as_moved": [line("then", [nan] + t1[1:] + t0, _binding7([((nan, 2, 3), (1, 1, 2), (0, 0, 0), 0.5), still]),
                                [nan] + t1[1:] + t0, _binding7([((nan, 2, 3), (1, 1, 2), (0, 0, 0), 0.5), still]))],
        # -0.0 == 0: unmoved when only the sign of a zero differs; moved elsewhere with a rot of -0.0 now, or then: flag 1, not 2
        "rot_minus_zero": [line("then", t0, _binding7([((1, 2, 3), (1, 1, 2), (-0.0, 0, 0), 0.5), ((1, 2, 3.5), (1, 1, 2), (0, -0.0, 0), 0.5),
                                                       ((1, 2, 3.5), (1, 1, 2), (0, 0, 0), 0.5)]),
                                t0, _binding7([still, still, ((1, 2, 3), (1, 1, 2), (0, 0, -0.0), 0.5)]))],
        "short_ellipsoid_buffer": [line("mark", t0, _binding7([still, rotated])[:-1]), line("mark", t0, _binding7([still], count=2)),
                                   line("then", t0, _binding7([still, rotated])[:-1], t0, _binding7([still, rotated])),
                                   line("then", t0, _binding7([still, rotated]), t0, _binding7([still, rotated])[:-1])],
        "odd_counts": [line("mark", t0, _binding7([still], count=c)) for c in (nan, -1.0, -0.5, 0.5, 1.5, 3e9, INF, -INF)] + [line("mark", t0, [])],
    }


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


# ------------------------------------------------------------------------------------------ the program
def _build(tmp, name, extra):
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "c", "image_args_check.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr      # no warning either
    return exe


def _run(exe, tmp, todo):
    """{name: lines} -> {name: answer lines}"""
    path = str(tmp / "scripts.txt")
    with open(path, "w") as f:
        for name, lines in todo.items():
            f.write("\n".join([f"script {name}"] + lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (exe, r.returncode, r.stderr[-2000:])
    out, cur = {}, None
    for line in r.stdout.splitlines():
        if line.startswith("== "):
            cur = out.setdefault(line[3:], [])
        else:
            cur.append(line)
    assert list(out) == list(todo)
    return out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("image_args")
    return tmp, [_build(tmp, "check_plain", []), _build(tmp, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def results(run, rows=None):
    """everything the golden file holds, computed by `run` ({name: lines} -> {name: answer lines}), and the rows and scripts it came from.  `rows`:
    the rows to generate the scripts from, when they are not to be `run`'s own"""
    rows = rows or parse_table(run({"table": ["table"]})["table"])
    scripts = scripts_of(rows)
    names = [row["name"] for row in rows]
    out = run({name: [scripts[name]["base"], scripts[name]["at_bounds"]] + [line for lines in scripts[name]["one"].values() for line in lines.values()]
               for name in names})
    base, at_bounds, one = {}, {}, {}
    for name in names:
        answers = iter(out[name])
        base[name] = next(answers)
        at_bounds[name] = [scripts[name]["at_bounds"], next(answers)]
        one[name] = {item: {v: next(answers) for v in lines} for item, lines in scripts[name]["one"].items()}
    pairs = pairs_of(rows, scripts, one)
    out = run({name: list(pairs[name].values()) for name in names})
    two = {name: dict(zip(pairs[name], out[name])) for name in names}
    packs = pack_scripts()
    messages = sorted({answer.split(" msg=", 1)[1] for name in names for answers in list(one[name].values()) + [two[name]] for answer in answers.values()})

    def short(answer):                                                # "rc msg" -> [rc, index of the message]
        rc, msg = answer.split(" msg=", 1)
        return [int(rc[3:]), messages.index(msg)]
    golden = dict(messages=messages, base=base, at_bounds=at_bounds, one={name: {item: {v: short(a) for v, a in answers.items()} for item, answers in one[name].items()} for name in names},
                  two={name: dict(n=len(two[name]), digest=digest([k + " " + a for k, a in two[name].items()])) for name in names}, pack=run(packs))
    return dict(golden=golden, rows=rows, scripts=scripts, one=one, pairs=pairs, two=two)


@pytest.fixture(scope="module")
def computed(programs):
    tmp, exes = programs

    def run_both(todo):
        outs = [_run(exe, tmp, todo) for exe in exes]
        assert outs[0] == outs[1]
        return outs[0]
    return results(run_both)


# ------------------------------------------------------------------------------------------ 1. equal to the parent
def test_answers_equal_what_the_scattered_checks_gave(computed):
    want = json.load(open(GOLDEN))
    got = computed["golden"]
    assert len(want["one"]) == 33 and sum(len(v) for item in want["one"].values() for v in item.values()) > 1400
    assert sum(t["n"] for t in want["two"].values()) > 2000
    for name in want["one"]:
        assert got["base"][name] == want["base"][name] == "rc=0 msg=", name
        for item in want["one"][name]:
            for v, (rc, m) in want["one"][name][item].items():
                assert (rc, got["messages"][got["one"][name][item][v][1]]) == (got["one"][name][item][v][0], want["messages"][m]), (name, item, v)
        assert got["two"][name] == want["two"][name], name
    assert all(answer == "rc=0 msg=" for _, answer in want["at_bounds"].values())
    for key_ in ("messages", "base", "at_bounds", "one", "two"):
        assert got[key_] == want[key_], key_


def test_packed_motion_records_equal_the_parents_bit_for_bit(computed):
    want = json.load(open(GOLDEN))["pack"]
    got = computed["golden"]["pack"]
    assert got == want and set(want) == set(pack_scripts())

    def f(line):
        d = dict(kv.split("=", 1) for kv in line.split())
        return int(d["nTri"]), int(d["nEl"]), [int(x) for x in d["triFlags"].split(",") if x], [int(x) for x in d["elFlags"].split(",") if x], d["tri"], d["el"]
    zero = "00000000" * 4
    assert f(got["nothing_mark"][0]) == f(got["nothing_then"][0]) == (0, 0, [], [], zero, zero)      # the one zero record
    assert f(got["mark"][0])[:4] == (3, 2, [0, 0, 0], [0, 0]) and len(f(got["mark"][0])[4]) == 3 * 12 * 8
    assert f(got["unmoved"][0])[:4] == (2, 2, [0, 0], [0, 0])
    assert f(got["flags"][0])[:4] == (3, 4, [0, 1, 1], [0, 1, 2, 2])
    assert f(got["beyond_the_mark"][0])[:4] == (3, 3, [0, 1, 1], [0, 1, 1])      # beyond the mark's count: moved, and no rot to undo
    assert f(got["beyond_the_mark"][1])[:4] == (1, 1, [0], [0])
    assert f(got["nan_counts_as_moved"][0])[:4] == (2, 2, [1, 0], [1, 0])
    assert f(got["rot_minus_zero"][0])[:4] == (1, 3, [0], [0, 1, 1])
    assert [f(line)[1] for line in got["short_ellipsoid_buffer"]] == [0, 0, 0, 2]
    assert f(got["short_ellipsoid_buffer"][2])[5] == zero and f(got["short_ellipsoid_buffer"][3])[3] == [1, 1]      # a mark of none: both are new
    assert [f(line)[1] for line in got["odd_counts"]] == [0, 0, 0, 0, 1, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------ 2. what the scripts reach
def test_rows_are_the_declared_functions(computed):
    names = [row["name"] for row in computed["rows"]]
    declared = sorted(n for h in IMAGE_HEADERS for n in _declared(h))
    assert len(names) == len(set(names)) == 33 and sorted(names) == sorted(declared + ["pt_render_adaptive"])
    assert "pt_render_adaptive" in _declared("pt_adaptive.h") and len(declared) == 32


def test_every_row_and_refusal_text_is_reached_and_every_bound_accepted(computed):
    accepted_somewhere = set()
    for row in computed["rows"]:
        name = row["name"]
        one, two = computed["one"][name], computed["two"][name]
        texts = [message(row, c) for c in row["checks"]]
        assert len(set(texts)) == len(texts), name
        said = {a.split(" msg=", 1)[1] for answers in one.values() for a in answers.values() if not a.startswith("rc=0 ")}
        assert said == set(texts), (name, said ^ set(texts))        # every refusal text of the row, and no other
        assert all(a.startswith("rc=-1 ") or a == "rc=0 msg=" for answers in one.values() for a in answers.values()), name
        # a pointer absent is always refused; a field at each bound passes the check that sets the bound
        pointers, fields, _ = items_of(row)
        assert all(one[p]["absent"].startswith("rc=-1 ") for p in pointers) and pointers[0] == "ctx", name
        for check in row["checks"]:
            for field, bs in bounds_of(check).items():
                for bound, nearest in bs:
                    answer = one[field][key(f32(nearest) if isinstance(nearest, float) else nearest)]
                    assert answer == "rc=0 msg=" or answer.split(" msg=", 1)[1] != message(row, check), (name, field, bound)
                    if answer == "rc=0 msg=":
                        accepted_somewhere.add((field, key(bound)))
                    # ... and the neighbour outside it does not (a bound at an infinity or at the end of int has none)
                    if isinstance(nearest, int):
                        outside = nearest + (1 if nearest == bs[1][1] else -1)
                        outside = outside if INT_MIN <= outside <= INT_MAX else None
                    else:
                        up = (bound, nearest) == bs[1]
                        with np.errstate(over="ignore"):
                            outside = f32(np.nextafter(np.float32(nearest), np.float32(INF if up else -INF)))
                        outside = None if outside == nearest or np.isnan(outside) else outside
                    if outside is not None and check["pred"] not in ("phase", "ordered"):
                        assert one[field][key(outside)].split(" msg=", 1)[1] == message(row, check), (name, field, bound)
        # both refused: the earlier check answers
        order = {t: k for k, t in enumerate(texts)}
        assert len(two) >= (len(pointers) + len(fields)) * (len(pointers) + len(fields) - 1) * 0.9, name
        for pair, answer in two.items():
            x, vx, y, vy = pair.split("|")
            mx, my = one[x][vx].split(" msg=", 1)[1], one[y][vy].split(" msg=", 1)[1]
            assert answer == "rc=-1 msg=" + min(mx, my, key=order.__getitem__), (name, pair)
    every = {(f, key(b)) for row in computed["rows"] for c in row["checks"] for f, bs in bounds_of(c).items() for b, _ in bs}
    assert accepted_somewhere == every
    # the texts without their prefixes: 3 of a null pointer, 7 int ranges, 6 "at least", 4 "> 0", 2 ">= 0", 3 of a floor, 5 float ranges, the ordered
    # pair, 2 of flags, the phase, the key
    texts = {c["text"] for row in computed["rows"] for c in row["checks"]}
    assert len(texts) == 35 and len({message(row, c) for row in computed["rows"] for c in row["checks"]}) == len(computed["golden"]["messages"]) - 1


def test_the_quirks_the_table_keeps(computed):
    rows = {row["name"]: row for row in computed["rows"]}

    def texts(name):
        return [message(rows[name], c) for c in rows[name]["checks"]]
    for name in ("pt_denoise_guided", "pt_read_display_denoised_guided", "pt_denoise_guided_demod", "pt_read_display_denoised_guided_demod"):
        assert texts(name)[0] == name + ": null argument" and texts(name)[-3:] == ["pt_denoise_guided: iterations must be in [0,8]", "pt_denoise_guided: min_frames must be >= 2",
                                                                                  "pt_denoise_guided: every sigma must be > 0 (+inf switches its term off)"], name
    assert texts("pt_reproject_frame_demod")[:3] == ["pt_reproject_frame_demod: null context", "pt_reproject_frame_demod: albedo_floor must be finite and > 0",
                                                     "pt_reproject_frame: max_history must be >= 1"]
    for name in ("pt_select_guided_demod", "pt_render_adaptive_guided_demod"):
        assert texts(name)[:2] == [name + ": albedo_floor must be finite and > 0", name + ": null argument"]
    for name in ("pt_fill_frame", "pt_fill_frame_through"):
        assert rows[name]["checks"][-1]["fields"] == ["sigma1", "sigma2", "sigma3"] and not any("iterations" in t or "min_frames" in t for t in texts(name))
    t = [c["text"] for c in rows["pt_reproject_frame_through"]["checks"]]
    assert t == ["null argument", "rule.radius must be in [0,4]", "rule.point_tol must be > 0", "null rule", "rule.max_depth must be in [0,8]",
                 "rule.min_weight must be in (0,1]", "rule.lobes must be in [0,3]", "unknown rule.flags",
                 "a rule that follows chains needs PT_THROUGH_KEY (the surface word is what a source is matched on)", "max_history must be >= 1", "depth_tol must be > 0",
                 "normal_tol must be in [-1, 1]", "unknown flags"]
    zero = key(0.0)
    assert computed["one"]["pt_reproject_frame_moved"]["albedo_floor"][zero] == "rc=0 msg="
    assert computed["one"]["pt_reproject_frame_demod"]["albedo_floor"][zero] == "rc=-1 msg=pt_reproject_frame_demod: albedo_floor must be finite and > 0"
    assert [c["text"].split(" must")[0] for c in rows["pt_select_guided"]["checks"][1:4]] == ["rule.iterations", "every sigma of the rule", "rule.min_frames"]


# ------------------------------------------------------------------------------------------ 3. a changed bound is seen
def test_a_changed_bound_fails_the_golden(programs, computed):
    tmp, _ = programs
    exe = _build(tmp, "check_iterations9", ["-DPT_ARGS_ITERATIONS_MAX=9"])
    got = results(lambda todo: _run(exe, tmp, todo), rows=computed["rows"])["golden"]
    want = json.load(open(GOLDEN))
    differ = [(name, item, v) for name in want["one"] for item in want["one"][name] for v in want["one"][name][item]
              if (got["one"][name][item][v][0], got["messages"][got["one"][name][item][v][1]]) != (want["one"][name][item][v][0], want["messages"][want["one"][name][item][v][1]])]
    takes_iterations = [row["name"] for row in computed["rows"] if any(c["fields"] == ["iterations"] for c in row["checks"])]
    # 9 is accepted now, and the text of the refusal names another range: nothing else moves
    assert len(takes_iterations) == 10
    assert differ == [(name, "iterations", v) for name in takes_iterations for v, (rc, _) in want["one"][name]["iterations"].items() if rc]
    assert all(want["one"][name]["iterations"]["9"][0] == -1 and got["one"][name]["iterations"]["9"][0] == 0 for name in takes_iterations)
    assert [name for name in want["two"] if got["two"][name] != want["two"][name]] == takes_iterations and got["pack"] == want["pack"]
