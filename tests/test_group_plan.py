"""CPU: the host-only plan of a group of streams (csrc/hip/pt_group_plan.hpp) through tests/c/group_plan_check.cpp, a stand-alone program built
twice with g++: plain, and under the address / undefined-behaviour sanitizers (which must stay silent and agree).

  * tile sharding against a short numpy model: every pixel in exactly one shard, tile-major, equal slot counts in whole blocks, -1 padding behind the
    pixels, one shard the identity, a part group the matching slice of the whole group's maps;
  * the shape of a group: every refusal text the header holds is reached, with its code, and nothing else is refused; the accepted shapes' runs,
    transport and streams per device;
  * the gather of one image, executed by the program on host arrays in every transport a shape allows (the program checks the result and the
    plan's properties; here its lines are held to what the shape implies)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pathtracer-0_amd", "csrc", "hip", "pt_group_plan.hpp")

SHARD_CASES = [(96, 40, 2), (100, 37, 3), (64, 64, 8), (100, 37, 16), (70, 41, 6), (160, 90, 4), (1920, 1080, 16), (32, 8, 2), (8, 4, 1)]


def _build(tmp, name, extra):
    exe = str(tmp / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "c", "group_plan_check.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("group_plan")
    return tmp, [_build(tmp, "check_plain", []), _build(tmp, "check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def _run_both(programs, args, outdirs=None):
    outs = []
    for k, exe in enumerate(programs[1]):
        a = [args[0], outdirs[k]] + args[1:] if outdirs else args
        r = subprocess.run([exe] + a, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stderr == "", (exe, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        outs.append(r.stdout.splitlines())
    assert outs[0] == outs[1]
    return outs[0]


def _model_pixels(W, H, rank, count):
    """the pixels of one shard: the 32 x 8 tiles in row-major order dealt round-robin, each tile's pixels row by row"""
    ntx, nty = -(-W // 32), -(-H // 8)
    px = []
    for t in range(rank, ntx * nty, count):
        ys, xs = np.arange(t // ntx * 8, min(H, t // ntx * 8 + 8)), np.arange(t % ntx * 32, min(W, t % ntx * 32 + 32))
        px.append((ys[:, None] * W + xs[None, :]).ravel())
    return np.concatenate(px) if px else np.zeros(0, np.int64)


def test_shard_maps_against_the_model(programs):
    # per case: the whole group; the same with five slots more; a part group in the middle (or the whole again, for one shard), and the last shard alone
    jobs = []
    for W, H, n in SHARD_CASES:
        mid = (n // 3, max(1, n // 2))
        jobs += [(W, H, n, 0, n, 0), (W, H, n, 0, n, 5), (W, H, n, mid[0], mid[1], 0), (W, H, n, n - 1, 1, 0)]
    dirs = []
    for k in range(2):
        dirs.append(str(programs[0] / f"maps{k}"))
        os.makedirs(dirs[-1], exist_ok=True)
    lines = _run_both(programs, ["shard"] + [str(v) for j in jobs for v in j], outdirs=dirs)
    assert len(lines) == len(jobs)
    got = []
    for k, (W, H, n, first, count, extra) in enumerate(jobs):
        m = re.match(rf"maps {k} slots=(\d+)$", lines[k])
        assert m, lines[k]
        a, b = (np.fromfile(os.path.join(d, f"{k}.bin"), np.int32) for d in dirs)
        assert np.array_equal(a, b) and a.size == count * int(m.group(1))
        got.append(a.reshape(count, int(m.group(1))))
    for c, (W, H, n) in enumerate(SHARD_CASES):
        whole, more, part, last = got[4 * c:4 * c + 4]
        model = [_model_pixels(W, H, r, n) for r in range(n)]
        slots = whole.shape[1]
        if n == 1:
            assert slots == W * H and np.array_equal(whole[0], np.arange(W * H))                      # one shard: the identity
            assert np.array_equal(more[0], np.concatenate([np.arange(W * H), np.full(5, -1)]))      # ... and -1 beyond W * H
        else:
            assert slots % 256 == 0 and slots == -(-max(len(p) for p in model) // 256) * 256, (W, H, n)
            for r in range(n):
                assert np.array_equal(whole[r, :len(model[r])], model[r]), (W, H, n, r)             # tile-major, as the model
                assert (whole[r, len(model[r]):] == -1).all()                                       # the padding follows the pixels
            assert more.shape[1] == slots + 5 and np.array_equal(more[:, :slots], whole) and (more[:, slots:] == -1).all()
        owned = whole[whole >= 0]
        assert np.array_equal(np.sort(owned), np.arange(W * H)), (W, H, n)                          # every pixel in exactly one shard
        first, count = jobs[4 * c + 2][3:5]
        assert np.array_equal(part, whole[first:first + count]) and np.array_equal(last, whole[n - 1:])      # a part group: the matching slice
    assert any(len(_model_pixels(W, H, n - 1, n)) == 0 for W, H, n in SHARD_CASES)                  # (32, 8, 2): a shard that owns no pixel
    assert min(len(_model_pixels(100, 37, r, 16)) for r in range(16)) <= 32 * 8                     # (100, 37, 16): shards of a single tile


# what the accepted shapes must come out as: runs (device, first, count), the collective, virtual devices, the group's streams on each stream's GPU
SHAPES = {
    "one": ([(0, 0, 1)], False, False, [1]),
    "two": ([(0, 0, 2)], False, False, [2, 2]),
    "three": ([(0, 0, 3)], False, False, [3, 3, 3]),
    "devices3": ([(0, 0, 1), (1, 1, 1), (2, 2, 1)], True, False, [1, 1, 1]),
    "pairs": ([(0, 0, 2), (1, 2, 2)], True, False, [2, 2, 2, 2]),
    "virtual4k2": ([(0, 0, 2), (0, 2, 2)], True, True, [4] * 4),
    "virtual16k8": ([(0, 2 * v, 2) for v in range(8)], True, True, [16] * 16),
    "forced": ([(0, 0, 1)], True, False, [1]),
    "part": ([(0, 0, 2)], False, False, [2, 2]),
    "virtual_k1": ([(0, 0, 2)], False, False, [2, 2]),
    "virtual_negative": ([(0, 0, 2)], False, False, [2, 2]),
    "two_no_queues": ([(0, 0, 2)], False, False, [2, 2]),
    "devices3_no_queues": ([(0, 0, 1), (1, 1, 1), (2, 2, 1)], True, False, [1, 1, 1]),
    "sixtyfour": ([(0, 0, 64)], False, False, [64] * 64),
}
ARG, ADJACENT = "pt_create_multi: bad argument", "pt_create_multi: the entries of one device must be adjacent ({0,0,1,1}, not {0,1,0,1})"
EQUAL, RANGE = "pt_create_multi: every device must be listed the same number of times", "pt_create_multi: HIP device index out of range"
VIRTUAL = "PT_MULTI_VIRTUAL_DEVICES=k needs ONE device listed a multiple of k times"
REFUSED = {
    "interleaved": (-1, ADJACENT), "uneven": (-1, EQUAL), "virtual3k2": (-1, VIRTUAL), "virtual_two_devices": (-1, VIRTUAL),
    "device_beyond": (-2, RANGE), "device_negative": (-2, RANGE), "part_beyond": (-1, ARG),
    "null_out": (-1, ARG), "null_devices": (-1, ARG), "none": (-1, ARG), "too_many": (-1, ARG), "width": (-1, ARG), "height": (-1, ARG),
    "first_negative": (-1, ARG), "total_short": (-1, ARG), "map_too_small": (-1, "pt_shard_map: n_slots too small"),
}


def test_group_shapes_and_every_refusal_text(programs):
    lines = _run_both(programs, ["shapes"])
    assert lines[-1] == "0 failures" and not any(ln.startswith("FAILED") for ln in lines)
    got, shapes = {}, {}
    for ln in lines:
        m = re.match(r"refusal (\w+) rc=(-?\d+) ?(.*)$", ln)
        if m:
            got[m.group(1)] = (int(m.group(2)), m.group(3))
        m = re.match(r"shape (\w+) runs=(\S+) rccl=(\d) virtual=(\d) sod=(\S+) warn=(\d)$", ln)
        if m:
            runs = [tuple(int(v) for v in r.split(":")) for r in m.group(2).split(",")]
            shapes[m.group(1)] = (runs, m.group(3) == "1", m.group(4) == "1", [int(v) for v in m.group(5).split(",")], m.group(6) == "1")
    # the header's texts, each reached with its code, and no other text
    texts = re.findall(r'Refused\{(PT_ERR_\w+),\s*"([^"]+)"\}', open(HEADER).read())
    assert len(texts) == 6
    codes = {"PT_ERR_ARG": -1, "PT_ERR_NO_DEVICE": -2}
    reached = set(got.values())
    for code, text in texts:
        assert (codes[code], text) in reached, text
    assert {t for _, t in reached if t} == {t for _, t in texts}
    # what is refused and what is not, by name, against the literal texts
    assert {k: v for k, v in got.items() if v[0]} == REFUSED
    assert set(got) == set(REFUSED) | set(SHAPES) and set(shapes) == set(SHAPES)
    for name, want in SHAPES.items():
        assert got[name] == (0, "") and shapes[name][:4] == want, name
        assert shapes[name][4] == (name == "two_no_queues"), name      # the warning: streams share a GPU and GPU_MAX_HW_QUEUES is not set


def test_gather_plans_executed_on_host_arrays(programs):
    lines = _run_both(programs, ["gather"])
    assert lines[-1] == "0 failures" and not any(ln.startswith("FAILED") for ln in lines)
    seen = set()
    for ln in lines[:-1]:
        m = re.match(r"gather (\w+) mode=(\w+) slots=(\d+) runs=(\d+) staging=(\S+) copies=(\d+) waits=(\d+) releases=(\d+) sends=(\d+) fromImage=(\d+) total=(\d+) untile=(\d)$", ln)
        assert m, ln
        name, mode, slots = m.group(1), m.group(2), int(m.group(3))
        staging = [int(v) for v in m.group(5).split(",")]
        copies, waits, releases, sends, from_image, total, untile = (int(m.group(k)) for k in range(6, 13))
        runs, rccl, virtual, sod = SHAPES[name]
        n, per = len(sod), runs[0][2]
        assert int(m.group(4)) == len(runs) and total == n * slots and untile == (name != "part"), ln
        if mode == "copies":      # one run, no send: the block is the gathered buffer
            assert len(runs) == 1 and staging == [0] and (copies, waits, releases, sends, from_image) == (n, n - 1, int(n > 1), 0, 0), ln
        elif per == 1:            # a one-stream run under the collective has no staging and sends its image
            assert staging == [0] * len(runs) and (copies, waits, releases, sends, from_image) == (0, 0, 0, len(runs), len(runs)), ln
        else:
            assert staging == [per * slots * 16] * len(runs) and (copies, waits, releases, sends, from_image) == (n, n - len(runs), len(runs), len(runs), 0), ln
        assert mode != "virtual" or virtual, ln
        seen.add((name, mode, slots))
    # every accepted shape, in each transport it allows, at both sizes
    want = set()
    for name, (runs, rccl, virtual, sod) in SHAPES.items():
        modes = ["copies", "rccl"] if len(runs) == 1 else ["rccl", "virtual"] if virtual else ["rccl"]
        want |= {(name, mode, slots) for mode in modes for slots in (256, 768)}
    assert seen == want
