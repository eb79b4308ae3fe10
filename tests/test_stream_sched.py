"""CPU: the frame-stream scheduler (csrc/hip/pt_stream_sched.hpp) through tests/c/stream_sched_check.cpp, a stand-alone program that runs scripts of
submissions against a deterministic model of the device and prints every action the scheduler asks of it.  Built twice with g++: plain, and under the
address / undefined-behaviour sanitizers (which must stay silent on every script, and agree).

  * every trace equals what the scheduler did before it was lifted out of pt_hip.hip (tests/golden/stream_sched_parent.json, recorded from that
    commit's own lines: see its "recorded" entry): the whole trace for two dozen named scripts, one digest per script family for all of them;
  * properties of every trace that need no golden: retirement in frame order, every batch retired exactly once by the time a synchronous call
    returns, at most two groups in flight (one in the tail) and one scan, no launch over more slots than the pool has, the iteration counter and the
    group sequence number wrapping as they should;
  * every decision of the scheduler is reached, under both ways a snapshot can land;
  * a build with one constant changed (groups of 16 iterations instead of 24) is seen by the golden traces.

One decision cannot be reached by calls alone: a scan whose first batch is no longer the front of the queue (see "stale_scan" in the program's
header for why).  The guard is kept as it was; the scripts reach it by moving the scan's word, in the recorder and here alike."""
import hashlib
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stream_sched_parent.json")
BRANCHES = ("new_stream", "join", "refuse_dirty", "refuse_inputs", "refuse_ring", "refuse_contract", "refuse_jobs", "ring_wait", "ring_restart", "pool_grown",
            "pool_kept", "kick_first", "issued_left", "issued_kick", "tail_group", "stale_epoch", "all_dead", "scan_partial", "scan_eight", "scan_moved",
            "discarded", "until_image", "until_ring", "dropped", "did_not_drain")      # SchedBranch, in its order
MODES = ("eager", "lazy")


# ------------------------------------------------------------------------------------------ the scripts
def submits(n, frames, first=1, inputs=1, asyn=1):
    return [f"submit {first + i * frames} {frames} {asyn} {inputs} 0 0" for i in range(n)]


def families():
    """{family: {script name: [lines]}}; every script under both landing modes (the name ends in the mode)"""
    fam = {}

    def add(family, name, create, lines):
        for mode in MODES:
            ppf, pool, life, seq0 = create
            fam.setdefault(family, {})[f"{name}|{mode}"] = [f"create {ppf} {pool} {life} {mode} 4 {seq0}"] + list(lines)

    # a fixed pool (pt_set_option 0): an asynchronous call comes back once the backlog is about one look's worth
    add("fixed", "basic", (100, 256, 3, 0), ["submit 1 2 0 1 0 0", "submit 3 4 1 1 0 0", "submit 7 4 1 1 0 0", "flush"])
    add("fixed", "long_jobs", (100, 256, 40, 0), submits(6, 16) + ["next_image", "submit 1 16 1 1 0 0", "finish_image 1", "flush"])
    add("fixed", "moved", (100, 128, 10, 0), submits(2, 1) + ["stale_scan"] + submits(6, 1, first=3) + ["flush"])
    # the automatic pool: a small one that grows with the backlog; an asynchronous call comes back at once
    add("refuse", "reasons", (100, 0, 40, 0), ["submit 1 2 1 1 0 0", "submit 3 2 1 1 1 0", "submit 5 2 1 2 0 0", "submit 7 2 1 2 0 1", "submit 9 20 1 2 0 1",
                                               "submit 29 2 1 2 0 1", "flush"])
    add("refuse", "jobs31", (1 << 20, 1 << 22, 1, 0), ["submit 1 1023 1 1 0 0"] * 3 + ["flush"])
    for life in (20, 41, 62, 76, 104, 132):          # whether the ring wait ends with rows free or with the stream over depends on when the batches finish
        add("ring", f"life{life}", (100, 0, life, 0), submits(5, 16) + ["flush"])
    add("ring", "megapixel", (1 << 20, 0, 6, 0), submits(6, 16) + ["next_image", "submit 1 16 1 1 0 0", "finish_image 1", "flush"])
    add("grow", "frame_by_frame", (1000, 0, 5, 0), submits(4, 1) + ["next_image"] + submits(2, 1) + ["finish_image 1", "flush"])
    add("grow", "eight", (64, 0, 60, 0), ["moments 1"] + submits(10, 1) + ["stale_scan"] + submits(2, 1, first=11) + ["next_image", "submit 1 3 1 1 0 0",
                                                                                                                        "finish_image 1", "flush"])
    # jobs that never end: the pump's bound, and the adaptive call's failure path
    add("never", "adaptive", (100, 256, 3, 0), ["submit 1 2 1 1 0 0", "never 1", "adaptive 3 2 50", "flush", "never 0", "submit 1 1 0 2 0 0", "adaptive 2 1 30",
                                                "never 1", "submit 3 1 0 2 0 0"])
    # the counters at their ends: the iteration number is 30 bits, the group sequence number 32 and never 0
    add("wrap", "both", (100, 256, 7, 0xfffffffa), ["submit 1 8 1 1 0 0", f"seek_iter {0x3fffffe8}"] + submits(3, 8, first=9) + ["flush"])
    add("wrap", "tail", (100, 512, 30, 0xfffffffe), ["submit 1 4 1 1 0 0", f"seek_iter {0x3ffffff8}", "flush", "submit 1 2 0 1 0 0"])
    # small scripts over pool x life x batch x pattern
    for pool in (128, 256, 1024, 4096, 0):
        for life in (1, 3, 10, 40):
            for frames in (1, 3, 8):
                add("sweep", f"async|{pool}|{life}|{frames}", (100, pool, life, 0), submits(5, frames) + ["flush"])
                add("sweep", f"mixed|{pool}|{life}|{frames}", (100, pool, life, 0), submits(2, frames) + submits(1, frames, first=50, asyn=0) + submits(2, frames, first=60) +
                    ["finish_image 0"])
                add("sweep", f"images|{pool}|{life}|{frames}", (100, pool, life, 0), submits(2, frames) + ["next_image"] + submits(2, frames) + ["next_image"] + submits(1, frames) +
                    ["finish_image 2", "finish_image 1", "next_image", "next_image", "flush"])
    return fam


NAMED = [f"{n}|{m}" for n in ("basic", "long_jobs", "moved", "reasons", "jobs31", "life62", "life76", "megapixel", "frame_by_frame", "eight", "adaptive", "both")
         for m in MODES]


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


# ------------------------------------------------------------------------------------------ the program
def _build(tmp, name, extra):
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "c", "stream_sched_check.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr      # no warning either
    return exe


def _run(exe, tmp, scripts):
    """{name: lines} -> {name: trace lines}"""
    path = str(tmp / "scripts.txt")
    with open(path, "w") as f:
        for name, lines in scripts.items():
            f.write("\n".join([f"script {name}"] + lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (exe, r.returncode, r.stderr[-2000:])
    out, cur = {}, None
    for line in r.stdout.splitlines():
        if line.startswith("== "):
            cur = out.setdefault(line[3:], [])
        else:
            cur.append(line)
    assert list(out) == list(scripts)
    return out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stream_sched")
    return tmp, [_build(tmp, "check_plain", []), _build(tmp, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def results(run):
    """everything the golden file holds, computed by `run` ({name: script lines} -> {name: trace lines}); the decisions reached are no part of a trace"""
    res = dict(traces={}, digests={}, all={}, reached={})
    for family, scripts in families().items():
        out = run(scripts)
        for name, lines in out.items():
            assert lines[-1].startswith("branches "), name
            res["reached"][name] = int(lines[-1].split()[1], 16)
            res["all"][name] = (scripts[name], lines[:-1])
            if name in NAMED:
                res["traces"][name] = lines[:-1]
        res["digests"][family] = digest([line for name in scripts for line in [name] + out[name][:-1]])
    assert set(NAMED) == set(res["traces"])
    return res


@pytest.fixture(scope="module")
def computed(programs):
    tmp, exes = programs

    def run_both(scripts):
        outs = [_run(exe, tmp, scripts) for exe in exes]
        assert outs[0] == outs[1]
        return outs[0]
    return results(run_both)


# ------------------------------------------------------------------------------------------ 1. equal to the parent
def test_traces_equal_what_the_scheduler_did_before_the_split(computed):
    want = json.load(open(GOLDEN))
    assert len(want["traces"]) >= 24
    for name in want["traces"]:
        assert computed["traces"][name] == want["traces"][name], name
    assert set(computed["traces"]) == set(want["traces"])
    assert computed["digests"] == want["digests"]


# ------------------------------------------------------------------------------------------ 2. properties
def fields(line):
    return dict(kv.split("=", 1) for kv in line.split()[1:] if "=" in kv)


CALLS = ("submit", "next_image", "finish_image", "flush", "adaptive")


def check_trace(name, script, trace):
    """walks a script and its trace together (the trace lines up to an "rc" line belong to one call); returns the calls' return codes"""
    calls = [line.split() for line in script[1:] if line.split()[0] in CALLS]
    seeks = any(line.startswith("seek_iter") for line in script)
    images, cur, seq = int(script[0].split()[5]), 0, int(script[0].split()[6])
    queue = []                           # batches submitted and not retired: (first frame, frames, image)
    in_flight, scans, pool, next_iter, last_f0, k, rcs = [], 0, 0, 0, -1, 0, []
    pumped = False                       # the call at hand had something to do: a submission, or batches to finish
    for line in trace:
        kind, f = line.split()[0], fields(line)
        call = calls[k]
        pumped = pumped or call[0] in ("submit", "adaptive") or bool(queue)
        if kind.startswith("rc="):
            rc = int(kind[3:])
            rcs.append(rc)
            if rc != 0:
                assert "error=" in line, (name, line)
                if call[0] == "adaptive":
                    queue = []                                    # the failed stream's batches are dropped
            elif call[0] == "next_image":
                cur = (cur + 1) % images
                assert all(q[2] != cur for q in queue), (name, line)      # nothing is still on its way into the image taken over
            elif call[0] == "finish_image":
                assert all(q[2] != (cur + images - int(call[1])) % images for q in queue), (name, line)
            elif call[0] != "submit" or call[3] == "0":
                assert queue == [], (name, line)                  # every batch has retired by the time a synchronous call returns
            if rc == 0 and pumped and (call[0] != "submit" or call[3] == "0"):
                assert in_flight == [], (name, line)              # synchronous callers leave no group behind them
            k, pumped = k + 1, False
            continue
        assert kind != "lost", (name, line)                       # no launch over fewer slots than are alive
        if kind == "init":
            assert queue == [], (name, line)                      # a new stream starts only once the last one has been flushed
            next_iter, last_f0 = 0, -1
        elif kind == "submit":
            pool = int(f["slots"])
            frames = int(call[2])
            assert int(f["jobs"]) == frames * (int(call[3]) if call[0] == "adaptive" else int(script[0].split()[1])), (name, line)
            queue.append((int(call[1]), frames, cur))
        elif kind == "group":
            assert 1 <= int(f["n"]) <= 24 and int(f["launched"]) <= pool, (name, line)      # never more slots than the pool has
            assert seeks or int(f["iter"]) == next_iter, (name, line)
            assert 0 <= int(f["iter"]) <= 0x3fffffff, (name, line)
            next_iter = (int(f["iter"]) + int(f["n"])) & 0x3fffffff
        elif kind == "snapshot":
            seq = (seq + 1) & 0xffffffff or 1
            assert int(f["seq"]) == seq != 0, (name, line)       # sequence 0 is never used
            assert int(f["inflight"]) == len(in_flight) <= (0 if f["tail"] == "1" else 1), (name, line)      # at most two in flight, one in the tail
            in_flight.append((seq, "scan" in f))
            scans += "scan" in f
            assert scans <= 1, (name, line)
        elif kind == "look":
            assert in_flight and in_flight[0][0] == int(f["seq"]), (name, line)      # snapshots are taken in the order of their launches
            scans -= in_flight.pop(0)[1]
        elif kind == "retire":
            assert queue and queue.pop(0) == (int(f["first"]), int(f["frames"]), int(f["image"])), (name, line)      # each once, oldest first
            assert int(f["f0"]) > last_f0, (name, line)          # in frame order
            last_f0 = int(f["f0"])
    assert k == len(calls), name
    return rcs


def test_properties_of_every_trace(computed):
    assert len(computed["all"]) > 300
    failed = 0
    for name, (script, trace) in computed["all"].items():
        rcs = check_trace(name, script, trace)
        failed += any(rcs)
        assert not any(rcs) or name.split("|")[0] == "adaptive", name      # the scripts that fail are the ones written to
    assert failed == len(MODES)
    # the counters wrap: the iteration number within 30 bits, the sequence number past 0xffffffff to 1
    for mode in MODES:
        trace = computed["all"][f"both|{mode}"][1]
        iters = [int(fields(line)["iter"]) for line in trace if line.startswith("group ")]
        seqs = [int(fields(line)["seq"]) for line in trace if line.startswith("snapshot ")]
        assert max(iters) > 0x3fffff00 and any(b < a for a, b in zip(iters, iters[1:]) if a > 0x3fffff00), mode
        assert 0xffffffff in seqs and seqs[seqs.index(0xffffffff) + 1] == 1, mode


def test_every_decision_is_reached_under_both_landing_modes(computed):
    for mode in MODES:
        reached = 0
        for name, bits in computed["reached"].items():
            if name.endswith("|" + mode):
                reached |= bits
        missing = [b for k, b in enumerate(BRANCHES) if not reached >> k & 1]
        assert missing == [], (mode, missing)
    # ... and where one would look for them
    def has(script, branch):
        return computed["reached"][script] >> BRANCHES.index(branch) & 1
    for mode in MODES:
        assert all(has(f"reasons|{mode}", b) for b in ("refuse_dirty", "refuse_inputs", "refuse_ring", "refuse_contract")) and has(f"jobs31|{mode}", "refuse_jobs")
        assert has(f"adaptive|{mode}", "dropped") and has(f"adaptive|{mode}", "did_not_drain")
        assert has(f"frame_by_frame|{mode}", "pool_grown") and has(f"frame_by_frame|{mode}", "pool_kept")
        assert has(f"eight|{mode}", "scan_eight")
    assert has("life76|eager", "ring_restart") and has("life62|eager", "ring_wait") and has("life62|lazy", "ring_wait") and has("life20|lazy", "ring_restart")


# ------------------------------------------------------------------------------------------ 3. a changed constant is seen
def test_a_changed_constant_fails_the_golden_traces(programs):
    tmp, _ = programs
    exe = _build(tmp, "check_group16", ["-DPT_SCHED_GROUP=16"])
    got = results(lambda scripts: _run(exe, tmp, scripts))
    want = json.load(open(GOLDEN))
    assert got["digests"] != want["digests"]
    assert got["traces"]["long_jobs|eager"] != want["traces"]["long_jobs|eager"]
    assert any(line.startswith("group n=24 ") for line in want["traces"]["long_jobs|eager"])
    assert not any(line.startswith("group n=24 ") for line in got["traces"]["long_jobs|eager"])
