"""CPU: the host-only planning of the intersect launches and of the pool's and the ring's sizes (csrc/hip/pt_launch_plan.hpp) through
tests/c/launch_plan_check.cpp, a stand-alone program built twice with g++: plain, and under the address / undefined-behaviour sanitizers (which must
stay silent on every case, and agree).

  * every plan equals, field for field, what the launch code decided before the split (tests/golden/launch_plan_parent.json, recorded from that
    commit's own lines: see its "recorded" entry): full lines for some 120 named cases, one digest per scene row for the whole cross product
    scene rows x option rows x device rows x launched; the pool, growth and ring sizes likewise;
  * properties of every plan that need no golden, and the magic divisor against integer division;
  * a build with one constant changed (the shared-GPU tile 8192 instead of 16384) is seen by the golden cases.

The cross product is taken whole.  The hand-made scene rows each change one thing of a base scene (4 BVHs, 14 stack levels, 16-bit stack entries), so that
a row says which input moved a plan.  (Deep trees are not crossed with wide entries: 64 levels of 4-byte entries under 1024-thread blocks of the compiled
kernel are 256 KB of stacks, which no CU has; the launch code never refused that combination of options, and the planner does not either.)"""
import hashlib
import itertools
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plan_parent.json")
LAYOUT_GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_layout_parent.json")
LDS_PER_CU = 160 * 1024

SCENE_FIELDS = ("nNodes", "nTriRecs", "numObj", "stackDepth", "stackMode", "asmNodeStride", "ellipMaps", "asmEligible", "ldsNodes", "ldsTris")
OPTION_FIELDS = ("extendMode", "extendTpb", "extendCacheBytes", "extendCacheSet", "extendMaxBlocksPerCU", "asmTpb", "asmLoop", "noneMin", "noneMinSet", "countStats")
DEVICE_FIELDS = ("numCUs", "streamsOnDevice", "part", "partEighths")
BASE_SCENE = dict(nNodes=3000, nTriRecs=3100, numObj=4, stackDepth=14, stackMode=0, asmNodeStride=80, ellipMaps=0, asmEligible=1, ldsNodes=112, ldsTris=0)
BASE_OPTIONS = dict(extendMode=2, extendTpb=256, extendCacheBytes=8192, extendCacheSet=0, extendMaxBlocksPerCU=0, asmTpb=0, asmLoop=-1, noneMin=8, noneMinSet=0,
                    countStats=0, probes=0, fast=0)


def scene_rows():
    layout = json.load(open(LAYOUT_GOLDEN))
    rows = {}
    for w in ("C1", "C2", "C3", "C4", "C5", "C6", "T1", "M1"):           # the workloads' numbers as the layout step builds them
        g = layout[w + "-default"]
        rows[w] = dict({k: int(g[k]) for k in SCENE_FIELDS if k != "nNodes"}, nNodes=int(g["nInner"]))
    hand = dict(base={}, fits_small_tile=dict(nNodes=40, nTriRecs=50, ldsNodes=40, ldsTris=50),      # 40 * 80 + 50 * 48 <= 8192
                bvh8=dict(numObj=8), bvh9=dict(numObj=9), bvh64=dict(numObj=64), bvh65=dict(numObj=65), bvh1024=dict(numObj=1024),
                depth1=dict(stackDepth=1), depth16=dict(stackDepth=16), depth32=dict(stackDepth=32), depth64=dict(stackDepth=64),
                mode1=dict(stackMode=1), mode2=dict(stackMode=2, nNodes=200000, nTriRecs=200100, asmNodeStride=64, ldsNodes=0), stride64=dict(asmNodeStride=64),
                no_large_blocks=dict(numObj=8, stackDepth=16),           # 8 * 4 + 16 * 2 = 64 B per lane: two 1024-thread blocks with 16 KB tiles exceed 160 KB
                refused_160k=dict(numObj=5000),                          # (5000 + 64) * 32 B of root records: fixed + 2048 > 160 KB
                ellip_maps=dict(ellipMaps=1), not_eligible=dict(asmEligible=0))
    for name, over in hand.items():
        rows[name] = dict(BASE_SCENE, **over)
    return rows


OPTION_ROWS = dict(
    default={}, asmTpb256=dict(asmTpb=256), asmTpb512=dict(asmTpb=512), asmTpb1024=dict(asmTpb=1024),
    tpb64=dict(extendTpb=64), tpb128=dict(extendTpb=128), tpb512=dict(extendTpb=512), tpb1024=dict(extendTpb=1024),
    cache0=dict(extendCacheBytes=0, extendCacheSet=1), cache2k=dict(extendCacheBytes=2048, extendCacheSet=1), cache64k=dict(extendCacheBytes=65536, extendCacheSet=1),
    cache150k=dict(extendCacheBytes=150 * 1024, extendCacheSet=1),
    blocks1=dict(extendMaxBlocksPerCU=1), blocks3=dict(extendMaxBlocksPerCU=3), blocks8=dict(extendMaxBlocksPerCU=8), blocks32=dict(extendMaxBlocksPerCU=32),
    loop0=dict(asmLoop=0), loop1=dict(asmLoop=1), noneMin5=dict(noneMin=5, noneMinSet=1), stats=dict(countStats=1),
    mode0=dict(extendMode=0), mode1=dict(extendMode=1), mode1_tpb1024_blocks3=dict(extendMode=1, extendTpb=1024, extendMaxBlocksPerCU=3),
    probes=dict(probes=1), fast=dict(fast=1), fast_asmTpb1024=dict(fast=1, asmTpb=1024))
DEVICE_ROWS = dict(alone=(256, 1, 0, 0), streams2=(256, 2, 0, 0), streams8=(256, 8, 0, 0), part3=(256, 1, 1, 3), part5=(256, 1, 1, 5), streams2_part3=(256, 2, 1, 3),
                   cu1=(1, 1, 0, 0))


def effective_cus(device):
    cus, _, part, eighths = device
    return cus * eighths // 8 if part else cus


def launched_row(device):
    full = effective_cus(device) * 2048
    return (1, 255, 256, 257, full - 1, full, 1 << 22, 1 << 23, 1 << 26)


def extend_cases(scenes):
    """{scene row: [(name, input line)]} over the whole cross product"""
    out = {}
    for sname, s in scenes.items():
        cases = []
        for (oname, over), (dname, dev) in itertools.product(OPTION_ROWS.items(), DEVICE_ROWS.items()):
            o = dict(BASE_OPTIONS, **over)
            for n in launched_row(dev):
                ints = [s[k] for k in SCENE_FIELDS] + [o[k] for k in OPTION_FIELDS] + list(dev) + [n, o["probes"], o["fast"]]
                cases.append((f"{sname}|{oname}|{dname}|{n}", "E " + " ".join(str(v) for v in ints), dict(scene=s, opt=o, dev=dev, launched=n)))
        out[sname] = cases
    return out


def named_cases(scenes):
    big = 1 << 22
    names = [f"{w}|default|{d}|{big}" for w in ("C1", "C2", "C3", "C4", "C5", "C6", "T1", "M1") for d in ("alone", "streams2")]
    names += [f"C3|{o}|alone|{big}" for o in OPTION_ROWS if o != "default"]
    names += [f"{s}|default|alone|{big}" for s in scenes if len(s) > 2]
    names += ["C3|default|part3|257", "C4|default|alone|524287", "C4|default|alone|524288", "C5|default|cu1|1", "refused_160k|default|streams2|256"]
    return names


JOBS = (1, 255, (1 << 20) - 1, (1 << 20) + 1, 1 << 22, (1 << 23) * 8 // 5 - 1, (1 << 23) * 8 // 5 + 1, (1 << 31) - 1)


def size_cases():
    """[(name, input line)]: the pool of a new stream, the growth of a running one, the ring"""
    new = [(f"new|{j}|{a}|{p}", f"N {j} {a} {p}") for j in JOBS for a in (0, 1) for p in (0, 1 << 21)]
    grow = [(f"grow|{j}|{img}|{alloc}|{act}", f"G {j} {img} {alloc} {act}") for j in JOBS for img in (0, 1 << 21, 1 << 24) for alloc in (1 << 23, 1 << 21)
            for act in (256, 1 << 20, (1 << 21) - 256, 1 << 22, (1 << 23) - 256, 1 << 23) if act <= alloc]
    # 8 GB / row bytes: 2^28-byte rows give 32 ring rows (fewer than 64), 2^20-byte rows 8192 (more)
    ring = [(f"ring|{n}|{a}|{rb}", f"R {n} {a} {rb} 4") for n in (1, 8, 100) for a in (0, 1) for rb in (1 << 28, 1 << 20, 16)]
    return new, grow, ring


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def launch_fields(line):
    """a plan line without perCU: what a launch shows (the golden was recorded from launches)"""
    return line[:line.index(" perCU=")]


# ------------------------------------------------------------------------------------------ the program
def _build(tmp, name, extra):
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "c", "launch_plan_check.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr      # no warning either
    return exe


def _run(exe, tmp, lines):
    path = str(tmp / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (exe, r.returncode, r.stderr[-2000:])
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("launch_plan")
    return tmp, [_build(tmp, "check_plain", []), _build(tmp, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def run_both(programs, lines):
    """the cases through both builds of the program: the same output, nothing on stderr, exit 0"""
    tmp, exes = programs
    outs = [_run(exe, tmp, lines) for exe in exes]
    assert outs[0] == outs[1]
    return outs[0]


def results(run, scenes=None):
    """everything the golden file holds, computed by `run` (input lines -> output lines)"""
    scenes = scenes or scene_rows()
    res = dict(plans={}, digests={}, all={})
    wanted = set(named_cases(scenes))
    for sname, cases in extend_cases(scenes).items():
        out = run([c[1] for c in cases])
        res["digests"][sname] = digest([launch_fields(o) if " perCU=" in o else o for o in out])
        for (name, _, inputs), o in zip(cases, out):
            if name in wanted:
                res["plans"][name] = launch_fields(o) if " perCU=" in o else o
            res["all"][name] = (inputs, o)
    assert wanted == set(res["plans"])
    new, grow, ring = size_cases()
    for key, cases in (("new", new), ("grow", grow), ("ring", ring)):
        out = run([c[1] for c in cases])
        res["digests"][key] = digest(out)
        if key != "grow":
            res["plans"].update({c[0]: o for c, o in zip(cases, out)})
        else:
            res["plans"].update({c[0]: o for c, o in zip(cases, out) if c[0].split("|")[2:] == ["0", str(1 << 23), str(1 << 20)]})
    return res


@pytest.fixture(scope="module")
def computed(programs):
    return results(lambda lines: run_both(programs, lines))


# ------------------------------------------------------------------------------------------ 1. equal to the parent
def test_plans_equal_what_the_launch_code_decided_before_the_split(computed):
    want = json.load(open(GOLDEN))
    assert len(want["plans"]) >= 36
    assert computed["plans"] == want["plans"]
    assert computed["digests"] == want["digests"]


# ------------------------------------------------------------------------------------------ 2. properties
def fields(line):
    return {k: int(v) for k, v in (kv.split("=") for kv in line.split())}


def test_properties_of_every_plan(computed):
    kernels = set()
    for name, (inp, line) in computed["all"].items():
        p, s, o, dev, launched = fields(line), inp["scene"], inp["opt"], inp["dev"], inp["launched"]
        kernels.add(p["kernel"])
        hand = p["kernel"] == 2
        cus = effective_cus(dev) if hand else dev[0]              # the partition's CUs are the hand-written kernel's; the compiled ones size their grid by the GPU
        ceil = -(-launched // p["tpb"])
        assert p["lds"] <= LDS_PER_CU and p["lds"] % 16 == 0, name
        assert p["ldsTris"] == 0 or p["ldsNodes"] == s["nNodes"], name
        assert 1 <= p["grid"] <= ceil, name
        if p["kernel"] != 0:                                      # persistent blocks: at most what is resident (k_extend: one block per 256 slots)
            assert p["grid"] <= cus * 2048 // p["tpb"], name
            assert p["grid"] == max(1, min(cus * p["perCU"], ceil)) and p["perCU"] >= 1, name
        if hand:
            assert p["nWaves"] == p["grid"] * p["tpb"] // 64 >= 1, name
            assert p["perCU"] * p["lds"] <= LDS_PER_CU, name
            contract = 1 if o["fast"] else 0
            base = {0: 0, 1: 1, 2: 4}[s["stackMode"]] + (1 if s["stackMode"] == 2 else 2) * contract
            assert p["variant"] == base + {256: 0, 1024: 6, 512: 12}[p["tpb"]] and 0 <= p["variant"] <= 17, name
            assert p["mode"] in (0, 1) and (o["asmLoop"] < 0 or p["mode"] == o["asmLoop"]), name
            m, sh, d = p["divM"], p["divS"], p["nWaves"]
            for x in (0, 1, d - 1, d, d + 1, launched, (1 << 31) - 1):
                assert (x * m >> 32) >> sh == x // d, name
            assert s["asmEligible"] and not o["countStats"] and o["extendTpb"] == 256 and o["extendMode"] == 2, name
        else:
            assert p["nWaves"] == 0 and p["variant"] == 0, name
            assert p["tpb"] == (o["extendTpb"] if p["kernel"] == 1 else 256), name
    assert kernels == {0, 1, 2}
    # the two refusals of the hand-written kernel fall to the compiled one
    assert fields(computed["all"][f"refused_160k|default|alone|{1 << 22}"][1])["kernel"] == 1
    assert fields(computed["all"][f"not_eligible|default|alone|{1 << 22}"][1])["kernel"] == 1
    assert fields(computed["all"][f"base|stats|alone|{1 << 22}"][1])["kernel"] == 1
    # a launch that gives every CU its two large blocks gets them, one slot short of it does not; never when two 16 KB tiles do not fit beside the stacks
    assert fields(computed["all"][f"base|default|alone|{256 * 2048}"][1])["tpb"] == 1024
    assert fields(computed["all"][f"base|default|alone|{256 * 2048 - 1}"][1])["tpb"] == 256
    assert fields(computed["all"][f"no_large_blocks|default|alone|{1 << 26}"][1])["tpb"] == 256


def test_magic_divisor_divides(programs):
    """mulhi(x, m) >> s == x / d for every x below 2^31"""
    ds = set(range(2, 4097))
    for k in range(1, 32):
        ds.update(d for d in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 2 <= d <= (1 << 31) - 1)
    ds = sorted(ds)
    top = (1 << 31) - 1
    for d, line in zip(ds, run_both(programs, [f"M {d}" for d in ds])):
        p = fields(line)
        assert p["m"] < 1 << 32
        for k in (2, 1000, top // d):
            for x in (0, 1, d - 1, d, d + 1, k * d - 1, k * d, top):
                if 0 <= x <= top:
                    assert (x * p["m"] >> 32) >> p["s"] == x // d, (d, x)


# ------------------------------------------------------------------------------------------ 3. a changed constant is seen
def test_a_changed_constant_fails_the_golden_cases(programs):
    tmp, _ = programs
    exe = _build(tmp, "check_tile8k", ["-DPT_PLAN_TILE_SHARED=8192"])
    got = results(lambda lines: _run(exe, tmp, lines))
    want = json.load(open(GOLDEN))
    assert got["plans"] != want["plans"] and got["digests"] != want["digests"]
    assert got["plans"][f"C3|default|streams2|{1 << 22}"] != want["plans"][f"C3|default|streams2|{1 << 22}"]
    assert got["plans"][f"C3|default|alone|{1 << 22}"] == want["plans"][f"C3|default|alone|{1 << 22}"]      # (alone on its GPU the tile is the other constant)
