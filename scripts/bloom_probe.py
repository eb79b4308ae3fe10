#!/usr/bin/env python3
"""The kernels of pt_tonemap_bloom beside k_tm_apply and k_display, and the filtered image taken on the device against its trip through the
host: profiles/r30_bloom.txt.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/bloom_probe.py --image c3|flat
        one context at 1920x1080; c3: one rendered C3 frame; flat: a written FRAME whose every pixel has the same colour.  Then ten
        pt_read_display_mean, ten pt_tonemap and ten pt_tonemap_bloom (6 levels) of FRAME, alternating.
    python scripts/bloom_probe.py --wall
        a rendered C3 image with moments, in one process: pt_denoise_guided to the host and pt_tonemap of that host image (the route without
        a device-resident source) against pt_read_display_denoised_guided and pt_tonemap_bloom of the filtered image at intensity 0 (the same
        picture), medians of ten, each call timed apart
    python scripts/bloom_probe.py --kernel-stats <dir> [--label text]
        the k_bl_*, k_tm_* and k_display rows of that run's *_kernel_stats.csv (device time), and the chain's sum per call
PT_HIP_LIB chooses another build of the library (an experiment on the kernels)."""
import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, CALLS, LEVELS = 1920, 1080, 10, 6


def _context(image, moments=False):
    import numpy as np
    import ptimport
    pt = ptimport.load()
    from pathtracer_0_amd import renderer
    r = renderer.Renderer(W, H)
    if image == "c3":
        r.load_workload(pt.scenes.build("C3", W, H))
        if moments:
            r.record_moments(True)
        r.reset_frame()
        r.render_batch(1, [pt.scenes.frame_seed(f) for f in range(1, 5 if moments else 2)])
    else:
        fr = np.empty((H, W, 4), np.float32)
        fr[...] = (0.5, 1.0, 0.25, 2.0)
        r.write_frame(fr)
    return r


def _median_ms(v):
    return 1e3 * sorted(v)[len(v) // 2]


def probe(image):
    r = _context(image)
    bloom = r.bloom_rule(levels=LEVELS, threshold=0.0 if image == "flat" else 1.0)      # flat: every pixel blooms
    wall = {"pt_read_display_mean": [], "pt_tonemap": [], "pt_tonemap_bloom": []}
    for _ in range(CALLS):
        t = time.perf_counter(); r.read_display_mean(java_bytes=False); wall["pt_read_display_mean"].append(time.perf_counter() - t)
        t = time.perf_counter(); plain = r.tonemap(); wall["pt_tonemap"].append(time.perf_counter() - t)
        t = time.perf_counter(); lit = r.tonemap_bloom(bloom=bloom); wall["pt_tonemap_bloom"].append(time.perf_counter() - t)
    print(f"{image}: exposure {lit[1]:.6g} (pt_tonemap's: {plain[1]:.6g}), {int((lit[0] != plain[0]).any(-1).sum())} of {W * H} pixels changed by the glare")
    for k, v in wall.items():
        print(f"wall ms, {k} (with its 6 MB read back): median {_median_ms(v):.3f}")
    r.close()


def wall():
    import numpy as np
    r = _context("c3", moments=True)
    zero = r.bloom_rule(intensity=0.0, levels=LEVELS)
    t = {"pt_denoise_guided to the host (33 MB down)": [], "pt_tonemap of that host image (33 MB up)": [],
         "pt_read_display_denoised_guided (6 MB down)": [], "pt_tonemap_bloom, filtered, intensity 0": [], "pt_tonemap_bloom, filtered, default rule": []}
    keys = list(t)
    for _ in range(CALLS):
        a = time.perf_counter(); X = r.denoise_guided(); b = time.perf_counter(); via_host = r.tonemap(X); c = time.perf_counter()
        r.read_display_denoised_guided(java_bytes=False); d = time.perf_counter(); on_device = r.tonemap_bloom("filtered", bloom=zero); e = time.perf_counter()
        r.tonemap_bloom("filtered"); f = time.perf_counter()
        for k, v in zip(keys, (b - a, c - b, d - c, e - d, f - e)):
            t[k].append(v)
        assert np.array_equal(via_host[0], on_device[0]) and via_host[1] == on_device[1]      # the same picture
    for k in keys:
        print(f"wall ms, {k}: median {_median_ms(t[k]):.3f}")
    print(f"wall ms, filter + display through the host: {_median_ms(t[keys[0]]) + _median_ms(t[keys[1]]):.3f};  on the device: {_median_ms(t[keys[2]]) + _median_ms(t[keys[3]]):.3f}")
    r.close()


def stats(d, label):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    assert files, d
    print(f"# {label}: name, calls, avg us, min us, max us")
    chain = 0.0
    for row in csv.DictReader(open(files[0])):
        n = row["Name"]
        if "k_bl_" in n or "k_tm_" in n or "k_display" in n:
            n = n[n.find("k_"):][:60]
            print("%s, %s, %.2f, %.2f, %.2f" % (n, row["Calls"], float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3))
            if "k_bl_" in n:
                chain += float(row["AverageNs"]) * int(row["Calls"]) / 1e3 / CALLS
    print("the bloom kernels of one call at %d levels (1 down_first, %d down, %d up, 1 compose), us: %.2f" % (LEVELS, LEVELS - 1, LEVELS - 1, chain))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", choices=("c3", "flat"))
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.kernel_stats:
        stats(a.kernel_stats, a.label)
    elif a.wall:
        wall()
    else:
        probe(a.image)
