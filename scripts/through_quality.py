#!/usr/bin/env python3
"""What are the seen-through records (include/pt_through.h) worth?  T1, C3 and C6 at 1080p, one stream -> profiles/r15_through_quality.{txt,json}.

(a) time: pt_read_features_through at depth 4 (every variant below) against pt_read_features on the same build, alternated in one process, the
    records invalidated before every call (an ORIGIN upload of the same values): wall time around the call, read-back included; medians.
(b) quality: clamped (display-referred, clip to [0, 1]) and unclamped RMSE against a REF_FRAMES-frame reference with seeds of its own, of lattice
    images ((0, 0) of stride 2) after 4 / 16 / 64 frames and of full images after 1 / 4 / 16 frames, every image through the filled demodulated
    guided filter (defaults, sigma_albedo = +inf, renderer.ALBEDO_FLOOR) on the first-hit records and on the records of every variant:
    reflection at 0.8 with the key, the same without it, both lobes at 0.5 with the key.  Overall, over the pixels whose first hit is a metal
    (Pm = 1), over those that are transmissive (Tr > 0), and over the filled ones of each.
(c) at 16 lattice frames, per first-hit material: the share of the pixels and the clamped / unclamped RMSE under each set of records.
(d) --probe: five pt_read_features and pt_read_features_through calls on C3 and nothing else, to run under rocprofv3 --kernel-trace --stats.
    --kernel-stats CSV ... puts the rows of such runs into the report.

usage: through_quality.py [--kernel-stats CSV [CSV ...]] [--out-dir profiles] [--scenes T1 C3 C6]
       through_quality.py --probe"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from guided_quality import render_to  # noqa: E402
from interleaved_quality import errors, lattice_to, mean_of  # noqa: E402

W, H = 1920, 1080
REF_FRAMES = 512
SCENES = ("T1", "C3", "C6")
LATTICE_FRAMES = (4, 16, 64)
FULL_FRAMES = (1, 4, 16)
ROUNDS = 5
DEPTH = 4
INF = float("inf")
# label -> (min_weight, lobes, key)
VARIANTS = {"reflect 0.8 key": (0.8, 1, True), "reflect 0.8 no key": (0.8, 1, False), "both 0.5 key": (0.5, 3, True)}
FIRST = "first-hit"


def invalidate(r, wl):
    r.set_buffer(0, np.asarray(wl.buffers[0], np.float32))


def read_times(r, wl, rules):
    """(a): wall seconds of every round, per set of records"""
    calls = {FIRST: r.read_features}
    for label, rule in rules.items():
        calls[label] = (lambda rule=rule: r.read_features_through(rule))
    for fn in calls.values():                           # warm-up: allocations
        invalidate(r, wl)
        fn()
    out = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for label, fn in calls.items():
            invalidate(r, wl)
            r.synchronize()
            t0 = time.perf_counter()
            fn()
            out[label].append(time.perf_counter() - t0)
    return out


def regions(wl, first, on):
    mtl = np.asarray(wl.buffers[14], np.float32)
    me = int(mtl[0])
    recs = [mtl[me * m: me * m + me] for m in range((mtl.size - 1) // me)]
    mat = np.ascontiguousarray(first[..., 11]).view(np.int32)
    hit = np.ascontiguousarray(first[..., 7]).view(np.int32) >= 0
    metal = hit & np.isin(mat, [m for m, rec in enumerate(recs) if rec[25] == 1])
    glass = hit & np.isin(mat, [m for m, rec in enumerate(recs) if rec[12] > 0])
    reg = {"all": np.ones_like(hit), "metal": metal, "transmissive": glass, "filled": ~on, "filled metal": metal & ~on, "filled transmissive": glass & ~on}
    per = [("miss", ~hit)]
    for m, rec in enumerate(recs):
        per.append((f"material {m} (Tr {rec[12]:g}, Pm {rec[25]:g}, Pr {rec[26]:g})", hit & (mat == m)))
    return {k: v for k, v in reg.items() if v.any()}, [(k, v) for k, v in per if v.any()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--kernel-stats", nargs="+", default=[])
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--scenes", nargs="+", default=list(SCENES))
    a = ap.parse_args()
    import ptimport
    pt = ptimport.load()
    from pathtracer_0_amd import renderer
    seed = pt.scenes.frame_seed
    fl = renderer.ALBEDO_FLOOR
    if a.probe:
        wl = pt.scenes.build("C3", W, H)
        r = renderer.Renderer(W, H)
        r.load_workload(wl)
        rule = r.through_rule(DEPTH, 0.5, 3, True)
        for _ in range(5):
            invalidate(r, wl)
            r.read_features()
            r.read_features_through(rule)
        r.close()
        print("probe done")
        return
    res = {"W": W, "H": H, "ref_frames": REF_FRAMES, "albedo_floor": fl, "depth": DEPTH, "variants": {k: list(v) for k, v in VARIANTS.items()}, "scenes": {}}
    yy, xx = np.mgrid[0:H, 0:W]
    on = (xx % 2 == 0) & (yy % 2 == 0)
    for name in a.scenes:
        wl = pt.scenes.build(name, W, H)
        r = renderer.Renderer(W, H)
        r.load_workload(wl)
        rules = {label: r.through_rule(DEPTH, mw, lobes, key) for label, (mw, lobes, key) in VARIANTS.items()}
        sc = {"read_wall_s": read_times(r, wl, rules)}
        first = r.read_features()
        reg, per = regions(wl, first, on)
        sc["followed"] = {}
        for label, rule in rules.items():
            k = np.ascontiguousarray(r.read_features_through(rule)[..., 14]).view(np.int32)
            sc["followed"][label] = [int(v) for v in np.bincount(k.ravel(), minlength=DEPTH + 1)]
        sc["share"] = {k: float(v.mean()) for k, v in reg.items()}
        r.reset_frame()
        render_to(r, seed, 1, REF_FRAMES, base=5000)
        ref = mean_of(r.read_frame())
        filt = lambda rule: r.denoise_guided(sigma_albedo=INF, albedo_floor=fl, fill=True, through=rule)[..., :3].astype(np.float64)     # noqa: E731
        r.record_moments(True)
        for kind, counts, go in (("lattice", LATTICE_FRAMES, lattice_to), ("full", FULL_FRAMES, render_to)):
            r.reset_frame()
            done, rows = 0, {}
            for n in counts:
                go(r, seed, done + 1, n)
                done = n
                row = {}
                for label, rule in [(FIRST, None)] + list(rules.items()):
                    img = filt(rule)
                    row[label] = {k: errors(img, ref, None if k == "all" else v) for k, v in reg.items() if kind == "lattice" or "filled" not in k}
                    if kind == "lattice" and n == 16:
                        row[label]["per_material"] = [(k, float(v.mean()), errors(img, ref, v)) for k, v in per]
                rows[str(n)] = row
            sc[kind] = rows
        res["scenes"][name] = sc
        r.close()
        print(f"{name}: done", flush=True)
    for path_csv in a.kernel_stats:
        with open(path_csv) as f:
            res.setdefault("kernel_stats", []).extend(dict(row, run=os.path.basename(path_csv)) for row in csv.DictReader(f))
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "r15_through_quality.json"), "w") as f:
        json.dump(res, f, indent=1)
    labels = [FIRST] + list(VARIANTS)
    L = [f"seen-through records (include/pt_through.h), {W}x{H}, one stream; max_depth {DEPTH}; the (0, 0) lattice of stride 2; reference {REF_FRAMES} frames with "
         f"seeds of their own; every image through the filled demodulated guided filter (defaults, sigma_albedo +inf, albedo_floor {fl}); untuned; "
         "scripts/through_quality.py"]
    for name, sc in res["scenes"].items():
        t = sc["read_wall_s"]
        L.append(f"(a) {name}: wall of one read, records invalidated first, read-back included, medians of {ROUNDS} alternated rounds, ms: " +
                 ", ".join(f"{k} {1e3 * np.median(v):.2f}" for k, v in t.items()))
        L.append("    ratio to first-hit: " + ", ".join(f"{k} {np.median(v) / np.median(t[FIRST]):.2f}" for k, v in t.items() if k != FIRST))
        for k, v in t.items():
            L.append(f"    every round, {k}: " + ", ".join(f"{1e3 * x:.2f}" for x in v))
        L.append("    pixels by k (0 .. 4): " + "; ".join(f"{k} {v}" for k, v in sc["followed"].items()))
        L.append("    share of the pixels: " + ", ".join(f"{k} {100 * v:.2f} %" for k, v in sc["share"].items()))
        for kind in ("lattice", "full"):
            L.append(f"(b) {name}, {kind} images: RMSE clamped / unclamped")
            for n, row in sc[kind].items():
                for region in row[FIRST]:
                    if region == "per_material":
                        continue
                    L.append(f"    {int(n):3d} frames  {region:20s} " + "   ".join(f"{lb}: {row[lb][region][0]:.4f} / {row[lb][region][1]:.4f}" for lb in labels))
        L.append(f"(c) {name}, 16 lattice frames, per first-hit material: share; RMSE clamped / unclamped")
        row = sc["lattice"]["16"]
        for i, (label, share, _) in enumerate(row[FIRST]["per_material"]):
            L.append(f"    {label:44s} {100 * share:6.2f} %   " + "   ".join(f"{lb}: {row[lb]['per_material'][i][2][0]:.4f} / {row[lb]['per_material'][i][2][1]:.4f}"
                                                                          for lb in labels))
    for k in res.get("kernel_stats", []):
        kn = k.get("Name", k.get("KernelName", ""))
        if any(t in kn for t in ("k_through", "k_feature", "k_extend", "pt_extend", "k_frame_setup", "k_init_control")):
            L.append(f"(d) {k['run']}: " + ", ".join(f"{c}={k[c]}" for c in k if c in ("Name", "KernelName", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs")))
    with open(os.path.join(a.out_dir, "r15_through_quality.txt"), "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
