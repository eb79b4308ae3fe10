#!/usr/bin/env python3
"""Are the kernels of one .hip file the same code objects in two trees?

  kernel_text_diff.py TREE_A TREE_B pathtracer-0_amd/csrc/hip/pt_reproject.hip [--rename 'NAME IN A=NAME IN B' ...] [--show NAME]

Compiles the file of both trees for the device alone (the flags of pathtracer-0_amd/build.py, to assembly) and prints, per kernel of tree A: whether its
instruction stream and its kernel descriptor are identical in tree B, the difference in instruction count, and next_free_vgpr / next_free_sgpr /
private_segment_fixed_size (scratch) / group_segment_fixed_size (LDS) of both with the waves per SIMD that the VGPRs allow (512 registers per lane, granules of 8,
at most 8 waves).  Before the comparison a kernel's own mangled name, the numbers of its block labels and the comments are normalised away, nothing else:
kernel-argument offsets are part of the instructions and have to agree.  Kernels are matched by their demangled names without the argument list, e.g.
"k_reproject<true, false, ReprojMotion, float>"; --rename maps a kernel whose template signature changed.  --show prints a unified diff of one kernel.
CPU only; reads nothing but the two trees.  Exit status 0 when every kernel of A has an identical partner in B, else 1."""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
CXXFILT = "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S"]
RESOURCES = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def short_name(mangled):
    d = subprocess.run([CXXFILT if os.path.exists(CXXFILT) else "c++filt", mangled], capture_output=True, text=True).stdout.strip() or mangled
    depth = 0
    for i in range(len(d) - 1, -1, -1):      # cut the argument list: the parenthesis that closes last
        depth += (d[i] == ")") - (d[i] == "(")
        if depth == 0 and d[i] == "(":
            d = d[:i]
            break
    d = d.replace("(anonymous namespace)::", "")
    return d[5:] if d.startswith("void ") else d


def kernels(tree, rel):
    """{short name: (normalised instruction lines, descriptor lines, {resource: value})} of the kernels of tree/rel"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.check_call([HIPCC] + FLAGS + [os.path.join(tree, rel), "-o", out])
        lines = open(out).read().split("\n")
    desc = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            j = next(k for k in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[k])
            desc[m.group(1)] = [x.strip() for x in lines[i + 1:j]]
    res = {}
    for sym, d in desc.items():
        a = next(k for k, l in enumerate(lines) if l.startswith(sym + ":"))
        b = next(k for k in range(a, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[k]))
        labels, body = {}, []
        for l in lines[a + 1:b]:
            l = l.split(";")[0].rstrip()      # comments: whole lines and tails
            if not l.strip():
                continue
            l = l.replace(sym, "KERNEL")
            l = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".LBB_%d" % len(labels)), l)      # block labels, by first appearance
            body.append(l.strip())
        r = {}
        for x in d:
            m = re.match(r"\.amdhsa_(\w+)\s+(\S+)", x)
            if m and m.group(1) in RESOURCES:
                r[m.group(1)] = int(m.group(2), 0)
        res[short_name(sym)] = (body, d, r)
    return res


def n_instructions(body):
    return sum(1 for l in body if not l.endswith(":") and not l.startswith("."))


def table(r):
    v = r["next_free_vgpr"]
    return "VGPRs %3d  SGPRs %3d  scratch %d  LDS %5d  waves / SIMD %d" % (v, r["next_free_sgpr"], r["private_segment_fixed_size"], r["group_segment_fixed_size"],
                                                                        min(8, 512 // max(8, (v + 7) // 8 * 8)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a"); ap.add_argument("tree_b"); ap.add_argument("file", help="the .hip file, relative to both trees")
    ap.add_argument("--rename", action="append", default=[], metavar="A=B", help="kernel A of the first tree is kernel B of the second")
    ap.add_argument("--show", action="append", default=[], metavar="A", help="print the diff of this kernel of the first tree")
    args = ap.parse_args()
    rename = dict(x.split("=", 1) for x in args.rename)
    ka, kb = kernels(args.tree_a, args.file), kernels(args.tree_b, args.file)
    same = 0
    for name in sorted(ka):
        other = rename.get(name, name)
        body, d, r = ka[name]
        if other not in kb:
            print("%s\n    missing in %s%s" % (name, args.tree_b, "" if other == name else " as " + other))
            continue
        body2, d2, r2 = kb[other]
        ident = body == body2 and d == d2
        same += ident
        print("%s%s\n    %s, instructions %d -> %d (%+d)" % (name, "" if other == name else "  ->  " + other,
                                                          "identical" if ident else "DIFFERENT" + ("" if body != body2 else " (descriptor only)"),
                                                          n_instructions(body), n_instructions(body2), n_instructions(body2) - n_instructions(body)))
        print("    A: %s\n    B: %s" % (table(r), table(r2)))
        if name in args.show:
            sys.stdout.writelines(x + "\n" for x in difflib.unified_diff(body + d, body2 + d2, name, other, lineterm=""))
    extra = sorted(set(kb) - {rename.get(n, n) for n in ka})
    for name in extra:
        print("%s\n    only in %s: %s" % (name, args.tree_b, table(kb[name][2])))
    print("%d of %d kernels of %s identical in %s%s" % (same, len(ka), args.tree_a, args.tree_b, ", %d kernels only there" % len(extra) if extra else ""))
    return 0 if same == len(ka) and not extra else 1


if __name__ == "__main__":
    sys.exit(main())
