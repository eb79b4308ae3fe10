"""CPU: the option table (csrc/hip/pt_options.hpp) through tests/c/options_check.cpp, a stand-alone program that runs scripts of `set` calls on a
fresh Options and prints what every call answered and every member afterwards.  Built twice with g++: plain, and under the address /
undefined-behaviour sanitizers (which must stay silent on every script, and agree).

  * every answer equals what pt_set_option's switch gave before the table replaced it (tests/golden/options_parent.json, recorded from that
    commit's own lines: see its "recorded" entry): for every option number -1..23 and every value of GRID plus the row's own bounds and their
    neighbours, the code, the message, the dirty flag and every member; the named sequences likewise;
  * every accepted set and every refusal text of the table is reached, and a refused set leaves every member as it was;
  * the rows' names and numbers are renderer.OPTIONS, their defaults a fresh Options;
  * a build with one bound changed (option 2 one byte short of a CU's LDS) is seen by the golden grid."""
import ast
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "options_parent.json")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
K = 1024
GRID = (I64_MIN, -(1 << 31) - 1, -(1 << 31), -2, -1, 0, 1, 2, 3, 7, 8, 9, 32, 33, 63, 64, 65, 128, 255, 256, 257, 512, 1024,
        150 * K - 1, 150 * K, 150 * K + 1, 160 * K - 1, 160 * K, 160 * K + 1, (1 << 26) - 1, 1 << 26, (1 << 26) + 1, (1 << 31) - 1, 1 << 31, I64_MAX)
# the lowest and the highest value each option accepts, as include/pt_debug.h states them (5 and 17 take a list between them; 0 takes 0
# and [256, 2^26]); 12 and 13 are queries, 15 is unassigned
BOUNDS = {0: (0, 1 << 26), 1: (I64_MIN, I64_MAX), 2: (0, 160 * K), 3: (1, 64), 4: (0, 2), 5: (64, 1024), 6: (0, 150 * K), 7: (1, 64), 8: (0, 32), 9: (0, 8),
          10: (0, (1 << 31) - 1), 11: (-1, 2), 14: (-1, 1), 16: (0, 1), 17: (0, 1024), 18: (0, 2), 19: (-1, 1), 20: (0, 1), 21: (0, 7)}
LISTS = {5: (64, 128, 256, 512, 1024), 17: (0, 256, 512, 1024)}
QUERIES = (12, 13)
REBUILDS = (2, 6, 10, 11, 18, 19, 20)
OPTION_NUMBERS = tuple(range(-1, 24))


def accepted(option, value):
    """what include/pt_debug.h says the option takes"""
    if option not in BOUNDS:
        return False
    if option in LISTS:
        return value in LISTS[option]
    if option == 0:
        return value == 0 or 256 <= value <= 1 << 26
    return BOUNDS[option][0] <= value <= BOUNDS[option][1]


def grid_of(option):
    values = set(GRID)
    if option in BOUNDS:
        lo, hi = BOUNDS[option]
        values.update(v for v in (lo - 1, lo, hi, hi + 1) if I64_MIN <= v <= I64_MAX)
    return sorted(values)


# a value that is not the default, a refused one (option 1 refuses nothing), the default again: tests/test_gpu_options.py replays this on a live context
REPLAY_VALUES = {0: (257, 255, 0), 1: (1, None, 0), 2: (4096, 160 * K + 1, 20 * K), 3: (5, 0, 8), 4: (1, 3, 2), 5: (512, 100, 256), 6: (2048, -1, 8 * K), 7: (30, 65, 24),
                 8: (3, 33, 0), 9: (4, 9, 6), 10: (64, -1, (1 << 31) - 1), 11: (2, 3, -1), 14: (0, 2, -1), 16: (1, 2, 0), 17: (512, 128, 0), 18: (1, 3, 0), 19: (1, 2, -1),
                 20: (0, 2, 1), 21: (3, 8, 0)}
REPLAY = [f"set {o} {v}" for o, vals in REPLAY_VALUES.items() for v in vals if v is not None] + ["set -1 0", "set 15 1", "set 22 0", "set 12 0", "set 13 0"]

SEQUENCES = {
    "refused_after_accepted": ["set 2 4096", "set 2 -1", "set 7 30", "set 7 65", "set 17 512", "set 17 128", "set 5 64", "set 5 0", "set 99 1"],
    "set_flags_stay": ["set 3 5", "set 3 0", "set 6 2048", "set 6 -1", "set 4 1", "set 3 8", "set 6 8192"],
    "pool_rounds_up": ["set 0 257", "set 0 256", "set 0 255", "set 0 0", "set 0 67108863", "set 0 67108864", "set 0 67108865"],
    "cull_round_trip": ["set 20 0", "set 20 1", "set 20 0", "set 20 2", "set 20 1"],
    "dirty_sticks": ["set 4 1", "set 2 1024", "set 4 2", "set 7 0", "set 99 1", "set 12 0", "set 13 5", "set 19 1"],
    "bools": ["set 1 -5", "set 1 0", "set 1 9223372036854775807", "set 16 1", "set 16 2", "set 16 0"],
    "replay": REPLAY,
}


def scripts():
    """{script name: lines}: one script per (option, value) of the grid, then the sequences"""
    out = {f"grid|{o}|{v}": [f"set {o} {v}"] for o in OPTION_NUMBERS for v in grid_of(o)}
    out.update(SEQUENCES)
    return out


def fields(line):
    """an answer line -> (rc, query, dirty, [members], msg)"""
    head, msg = line.split(" msg=", 1)
    f = dict(kv.split("=", 1) for kv in head.split())
    return int(f["rc"]), int(f["query"]), int(f["dirty"]), [int(v) for v in f["fields"].split(",")], msg


def renderer_options():
    """renderer.OPTIONS read from the source: importing the module is the business of the GPU tests"""
    tree = ast.parse(open(os.path.join(ROOT, "pathtracer-0_amd", "renderer.py")).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and [getattr(t, "id", None) for t in node.targets] == ["OPTIONS"]:
            return ast.literal_eval(node.value)
    raise AssertionError("renderer.py has no OPTIONS")


# ------------------------------------------------------------------------------------------ the program
def _build(tmp, name, extra):
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "c", "options_check.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr      # no warning either
    return exe


def _run(exe, tmp, todo):
    """{name: lines} -> {name: answer lines}, and the lines of `fields` and `table` under "fields" and "table" """
    path = str(tmp / "scripts.txt")
    with open(path, "w") as f:
        for name, lines in todo.items():
            f.write("\n".join([f"script {name}"] + lines) + "\n")
        f.write("script fields\nfields\nscript table\ntable\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (exe, r.returncode, r.stderr[-2000:])
    out, cur = {}, None
    for line in r.stdout.splitlines():
        if line.startswith("== "):
            cur = out.setdefault(line[3:], [])
        else:
            cur.append(line)
    assert list(out) == list(todo) + ["fields", "table"]
    return out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("options")
    return tmp, [_build(tmp, "check_plain", []), _build(tmp, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def results(run):
    """everything the golden file holds, computed by `run`"""
    out = run(scripts())
    res = dict(fields=out["fields"][0], grid={}, sequences={name: out[name] for name in SEQUENCES}, table=out["table"])
    for o in OPTION_NUMBERS:
        res["grid"][str(o)] = {str(v): out[f"grid|{o}|{v}"][0] for v in grid_of(o)}
    return res


@pytest.fixture(scope="module")
def computed(programs):
    tmp, exes = programs

    def run_both(todo):
        outs = [_run(exe, tmp, todo) for exe in exes]
        assert outs[0] == outs[1]
        return outs[0]
    return results(run_both)


# ------------------------------------------------------------------------------------------ 1. equal to the parent
def test_answers_equal_what_the_switch_gave_before_the_table(computed):
    want = json.load(open(GOLDEN))
    assert computed["fields"] == want["fields"]
    assert set(want["grid"]) == {str(o) for o in OPTION_NUMBERS} and sum(len(g) for g in want["grid"].values()) >= len(OPTION_NUMBERS) * len(GRID)
    for o in want["grid"]:
        for v in want["grid"][o]:
            assert computed["grid"][o][v] == want["grid"][o][v], (o, v)
    assert computed["grid"] == want["grid"]
    assert computed["sequences"] == want["sequences"] and set(want["sequences"]) == set(SEQUENCES)


# ------------------------------------------------------------------------------------------ 2. what the grid reaches, and what a call may touch
def test_every_accepted_set_and_every_refusal_is_reached(computed):
    names = computed["fields"].split(",")
    assert len(names) == len(set(names)) == 21
    fresh = fields(computed["grid"]["12"]["0"])[3]
    refusals, stored = {}, {}
    for o in OPTION_NUMBERS:
        for v in grid_of(o):
            rc, query, dirty, members, msg = fields(computed["grid"][str(o)][str(v)])
            if o in QUERIES:                                          # the context answers them: the table stores nothing and refuses nothing
                assert (rc, query, dirty, msg) == (0, 1, 0, ""), (o, v)
                assert members == fresh, (o, v)
                continue
            assert query == 0 and (rc == 0) == accepted(o, v), (o, v)
            if rc:
                assert rc == -1 and msg and dirty == 0 and members == fresh, (o, v)      # PT_ERR_ARG; a refused call leaves every member as it was
                refusals.setdefault(o, set()).add(msg)
            else:
                assert msg == "" and dirty == (o in REBUILDS), (o, v)
                changed = [n for n, a, b in zip(names, fresh, members) if a != b]
                assert len([n for n in changed if not n.endswith("Set")]) <= 1, (o, v)      # one member, and its flag
                stored.setdefault(o, set()).add(tuple(members))
    # one text per option that can refuse, one for every number that is no option; 22 with the three only the context gives (a null context, the two queries)
    assert all(len(texts) == 1 for texts in refusals.values())
    assert sorted(refusals) == [-1, 0] + [o for o in range(2, 24) if o not in QUERIES]
    assert {o for o, t in refusals.items() if t == {"unknown option"}} == {-1, 15, 22, 23}
    assert len({t for texts in refusals.values() for t in texts}) == 19
    # every accepted value of the grid left a state of its own (option 1 keeps whether it was zero, option 0 whole blocks of 256 slots)
    for o in BOUNDS:
        values = [v for v in grid_of(o) if accepted(o, v)]
        assert len(stored[o]) == len({v != 0 for v in values} if o == 1 else {-(-v // 256) for v in values} if o == 0 else values), o
    for v in grid_of(0):
        if accepted(0, v):
            assert fields(computed["grid"]["0"][str(v)])[3][names.index("poolSlots")] == -(-v // 256) * 256, v


def test_sequences(computed):
    names = computed["fields"].split(",")

    def trace(name):
        return [(rc, dirty, dict(zip(names, members)), msg) for rc, _, dirty, members, msg in map(fields, computed["sequences"][name])]
    t = trace("refused_after_accepted")
    assert [rc for rc, *_ in t] == [0, -1, 0, -1, 0, -1, 0, -1, -1]
    assert t[1][2]["ldsBudget"] == 4096 and t[3][2]["refillMin"] == 30 and t[5][2]["asmTpb"] == 512 and t[7][2]["extendTpb"] == 64
    assert t[-1][2] == t[-2][2] and t[-1][3] == "unknown option"
    t = trace("set_flags_stay")
    assert [(m["noneMinSet"], m["extendCacheSet"]) for _, _, m, _ in t] == [(1, 0), (1, 0), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1)]
    assert t[-1][2]["noneMin"] == 8 and t[-1][2]["extendCacheBytes"] == 8192      # back at the default values, still the caller's
    t = trace("pool_rounds_up")
    assert [m["poolSlots"] for _, _, m, _ in t] == [512, 256, 256, 0, 1 << 26, 1 << 26, 1 << 26] and [rc for rc, *_ in t] == [0, 0, -1, 0, 0, 0, -1]
    t = trace("cull_round_trip")
    assert [m["asmNoRootCull"] for _, _, m, _ in t] == [1, 0, 1, 1, 0] and [rc for rc, *_ in t] == [0, 0, 0, -1, 0]
    t = trace("dirty_sticks")
    assert [dirty for _, dirty, _, _ in t] == [0, 1, 1, 1, 1, 1, 1, 1]      # raised by option 2, lowered by no later call, accepted, refused, unknown or a query
    t = trace("bools")
    assert [m["countStats"] for _, _, m, _ in t[:3]] == [1, 0, 1] and [m["fastContract"] for _, _, m, _ in t[3:]] == [1, 1, 0]
    t = trace("replay")
    fresh = dict(zip(names, fields(computed["grid"]["12"]["0"])[3]))
    assert 55 <= len(t) <= 65 and t[-1][2] == dict(fresh, noneMinSet=1, extendCacheSet=1)      # every default again, the two flags raised


# ------------------------------------------------------------------------------------------ 3. names and defaults
def test_rows_are_renderer_options_and_defaults_a_fresh_options(computed):
    rows = [line.split() for line in computed["table"]]
    assert {name: int(number) for number, name, *_ in rows} == renderer_options()
    assert [int(r[0]) for r in rows] == [o for o in range(22) if o != 15]
    assert {int(r[0]) for r in rows if r[2] == "query"} == set(QUERIES) and all(r[2] in ("query", "value") for r in rows)
    names = computed["fields"].split(",")
    fresh = dict(zip(names, fields(computed["grid"]["12"]["0"])[3]))
    assert fresh == dict(poolSlots=0, ldsBudget=20 * K, noneMin=8, extendMode=2, extendTpb=256, extendCacheBytes=8 * K, refillMin=24, extendMaxBlocksPerCU=0,
                         innerKeepEighths=6, bfsNodes=(1 << 31) - 1, stackModeForce=-1, asmLoop=-1, asmTpb=0, forceNiBits8=0, asmNodeLayout=-1, cuPartition=0,
                         countStats=0, noneMinSet=0, extendCacheSet=0, fastContract=0, asmNoRootCull=0)
    written = set()
    for number, name, kind, default, member in rows:
        if kind == "query":
            continue
        assert member in fresh and member not in written, name      # every row its own member
        written.add(member)
        assert int(default) == (1 - fresh[member] if name == "asm_root_cull" else fresh[member]), name
        assert accepted(int(number), int(default)) and int(default) == REPLAY_VALUES[int(number)][2], name
    assert set(names) - written == {"noneMinSet", "extendCacheSet"}


# ------------------------------------------------------------------------------------------ 4. a changed bound is seen
def test_a_changed_bound_fails_the_golden_grid(programs):
    tmp, _ = programs
    exe = _build(tmp, "check_lds_short", [f"-DPT_OPT_LDS_BUDGET_MAX={160 * K - 1}"])
    got = results(lambda todo: _run(exe, tmp, todo))
    want = json.load(open(GOLDEN))
    differ = [(o, v) for o in want["grid"] for v in want["grid"][o] if got["grid"][o][v] != want["grid"][o][v]]
    assert differ == [("2", str(160 * K))]
    assert got["sequences"] == want["sequences"]
