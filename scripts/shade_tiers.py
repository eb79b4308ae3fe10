#!/usr/bin/env python3
"""Static load-tier report of the shading kernel: compiles csrc/hip/pt_hip.hip for gfx950 (device code only, no GPU needed) and prints, for
every k_shade instantiation, its vector-memory load tiers, VGPRs, waves per SIMD and scratch bytes, and (--json, and the last column) how many of
round trips on path-state groups a wave waits out before the kernel's first s_barrier, that of the block's job pull (pre_barrier_trips, see pre_barrier).

usage: shade_tiers.py [--json] [--asm FILE]      (--asm: read an already compiled .s instead of compiling)

A tier is a run of vector loads (global_load*, and atomics that return a value) ended by an s_waitcnt on vmcnt; a wait that follows no new
load ends no tier.  The count walks the kernel's code in layout order, so a load on a branch that a given lane does not take still counts:
it is an upper bound on the round trips one wave waits out one after another, and it rises whenever an edit serialises a load behind the
wait of another.  Waves per SIMD follow from the VGPR allocation (granule 8, 512 per SIMD lane, at most 8 waves)."""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pathtracer-0_amd", "csrc", "hip", "pt_hip.hip")
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]
# the assembled intersect kernels are not needed to compile the device code: empty arrays of the same names stand in for them
ASM_VARIANTS = [n + w for w in ("", "w", "h") for n in ("s16", "p18", "s16f", "p18f", "p24", "p24f")]
LOAD = re.compile(r"^\s*(global_load|buffer_load|flat_load|global_atomic\S*.*\bsc0\b|buffer_atomic\S*.*\bsc0\b)")
WAIT = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\(")
STATE_LOAD = re.compile(r"^\s*global_load_dwordx[24]\b")
VMCNT = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\((\d+)\)")
BARRIER = re.compile(r"^\s*s_barrier\b")
KNAME = re.compile(r"^(_ZN12_GLOBAL__N_17k_shadeILi(\d+)ELb([01])ELb([01])ELb([01])ELb([01])E\S*):(\s|$)")


def compile_asm(out_dir):
    inc = os.path.join(out_dir, "stub.inc")
    with open(inc, "w") as f:
        f.writelines(f"static const unsigned char pt_extend_hsaco_{n}[1] = {{0}};\n" for n in ASM_VARIANTS)
    out = os.path.join(out_dir, "pt_hip.s")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    subprocess.run([hipcc] + HIP_FLAGS + ["--cuda-device-only", "-S", f'-DPT_EXTEND_INC="{inc}"', SRC, "-o", out],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


def tiers(body):
    n, pending = 0, False
    for line in body:
        if LOAD.match(line):
            pending = True
        elif pending and WAIT.match(line):
            n, pending = n + 1, False
    return n


def pre_barrier(body):
    """The round trips on path-state groups that the code laid out before the first s_barrier waits out one after another.  A state group is
    read 8 or 16 bytes per lane (STATE_LOAD); the 4-byte read of the tail's dense queue, which a launch outside the tail branches around, is
    not one.  vmcnt counts loads in issue order, so `vmcnt(N)` after k loads has waited for the first k - N of them: a wait is a new trip only
    if it waits for a load issued after the previous trip ended.  (A wait for an older load, which was in flight during that trip already,
    costs no further round trip: the first tier's `vmcnt(2)`, load, `vmcnt(2)`, `vmcnt(1)` is one trip, not three.)"""
    issued = mark = trips = 0
    for line in body:
        if BARRIER.match(line):
            break
        if STATE_LOAD.match(line):
            issued += 1
            continue
        m = VMCNT.match(line)
        if m and issued - int(m.group(1)) > mark:
            trips, mark = trips + 1, issued
    return trips


def report(asm_text):
    lines = asm_text.splitlines()
    out = {}
    for k, line in enumerate(lines):
        m = KNAME.match(line)
        if not m:
            continue
        sym = m.group(1)
        end = next(j for j in range(k, len(lines)) if lines[j].startswith(".Lfunc_end"))
        at = next(j for j in range(len(lines)) if lines[j].strip() == f".amdhsa_kernel {sym}")
        desc = "\n".join(lines[at:at + 80])
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1))
        name = "k_shade<%s,%s>" % (m.group(2), ",".join("true" if b == "1" else "false" for b in m.group(3, 4, 5, 6)))
        out[name] = dict(tiers=tiers(lines[k:end]), vgpr=vgpr, waves_per_simd=min(8, 512 // (-(-vgpr // 8) * 8)), scratch_bytes=scratch,
                         pre_barrier_trips=pre_barrier(lines[k:end]))
    return out


def main():
    args = sys.argv[1:]
    if "--asm" in args:
        text = open(args[args.index("--asm") + 1]).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            text = open(compile_asm(d)).read()
    r = report(text)
    if "--json" in args:
        print(json.dumps(r, indent=1, sort_keys=True))
        return
    print(f"{'kernel (STK, STATS, DIRECT, TEX, FAST)':44s} tiers  vgpr  waves/SIMD  scratch  pre-barrier")
    for name in sorted(r, key=lambda s: [int(x) if x.isdigit() else x for x in re.split(r"(\d+)", s)]):
        v = r[name]
        print(f"{name:44s} {v['tiers']:5d} {v['vgpr']:5d} {v['waves_per_simd']:11d} {v['scratch_bytes']:8d} {v['pre_barrier_trips']:12d}")


if __name__ == "__main__":
    main()
