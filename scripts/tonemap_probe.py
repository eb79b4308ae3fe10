#!/usr/bin/env python3
"""The kernels of pt_tonemap beside k_display, which moves the same bytes (16 B in, 3 B out per pixel): profiles/r27_tonemap.txt.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/tonemap_probe.py --image c3|flat
        one context at 1920x1080; c3: one rendered C3 frame; flat: a written FRAME whose every pixel has the same colour (every luminance in
        one bin: the histogram's worst case).  Then ten pt_read_display_mean and ten pt_tonemap of FRAME with the histogram, alternating.
    python scripts/tonemap_probe.py --kernel-stats <dir> [--label text]
        the k_tm_* and k_display rows of that run's *_kernel_stats.csv (device time)
PT_HIP_LIB chooses another build of the library (an experiment on the kernels)."""
import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, CALLS = 1920, 1080, 10


def probe(image):
    import numpy as np
    import ptimport
    pt = ptimport.load()
    from pathtracer_0_amd import renderer
    r = renderer.Renderer(W, H)
    if image == "c3":
        r.load_workload(pt.scenes.build("C3", W, H))
        r.reset_frame()
        r.render_batch(1, [pt.scenes.frame_seed(1)])
    else:
        fr = np.empty((H, W, 4), np.float32)
        fr[...] = (0.5, 1.0, 0.25, 2.0)
        r.write_frame(fr)
    wall = {"pt_read_display_mean": [], "pt_tonemap": []}
    for _ in range(CALLS):
        t = time.perf_counter(); r.read_display_mean(java_bytes=False); wall["pt_read_display_mean"].append(time.perf_counter() - t)
        t = time.perf_counter(); rgb, e, hist = r.tonemap(want_hist=True); wall["pt_tonemap"].append(time.perf_counter() - t)
    print(f"{image}: exposure {e:.6g}, {int((hist > 0).sum())} bins in use, the fullest holds {int(hist.max())} of {W * H} pixels")
    for k, v in wall.items():
        print(f"wall ms, {k} (with its 6 MB read back): median {1e3 * sorted(v)[len(v) // 2]:.3f}")
    r.close()


def stats(d, label):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    assert files, d
    print(f"# {label}: name, calls, avg us, min us, max us")
    for row in csv.DictReader(open(files[0])):
        n = row["Name"]
        if "k_tm_" in n or "k_display" in n:
            n = n[n.find("k_"):][:60]
            print("%s, %s, %.2f, %.2f, %.2f" % (n, row["Calls"], float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", choices=("c3", "flat"))
    ap.add_argument("--kernel-stats")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.kernel_stats:
        stats(a.kernel_stats, a.label)
    else:
        probe(a.image)
