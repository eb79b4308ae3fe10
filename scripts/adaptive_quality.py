#!/usr/bin/env python3
"""Adaptive sampling (include/pt_adaptive.h) on C3, one GPU, one stream: throughput against the active fraction, and image error at equal wall time.

  reference  a high-spp uniform image (--ref-frames frames x SAMPLE_RES spp, seeds disjoint from the runs below)
  uniform    pt_render_batch in chunks of --chunk frames; per chunk: time, per-pixel RMSE of FRAME.rgb / FRAME.a against the reference
  adaptive   pt_render_adaptive: --chunk frames for every pixel (min_frames), then calls of --chunk frames on the pixels the rule keeps,
             for every rel_err of --rel; per call: active fraction, time, Msamples/s, RMSE
The equal-time comparison interpolates the uniform RMSE-versus-time curve at each adaptive checkpoint's elapsed time.  Times are wall times of the
synchronous calls (pt_synchronize included), the read-backs for the RMSE are not timed.

usage: adaptive_quality.py [--W 1920 --H 1080] [--ref-frames 512] [--frames 64] [--chunk 4] [--rel 0.05,0.02,0.01] [--out profiles/x.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ptimport  # noqa: E402

pt = ptimport.load()
from pathtracer_0_amd import renderer, scenes  # noqa: E402


def rmse(F, ref_mean):
    with np.errstate(all="ignore"):
        m = F[..., :3] / F[..., 3:4]
    d = (m.astype(np.float64) - ref_mean)
    ok = np.isfinite(d).all(axis=2)
    return float(np.sqrt(np.mean(d[ok] ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--ref-frames", type=int, default=512)
    ap.add_argument("--frames", type=int, default=64, help="frames of the uniform run")
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--rel", default="0.05,0.02,0.01")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H, K = a.W, a.H, a.chunk
    wl = scenes.build("C3", W, H)
    spp = int(wl.sample_res)
    r = renderer.Renderer(W, H)
    r.load_workload(wl)
    seed = lambda f: scenes.frame_seed(f)                       # noqa: E731
    ref_seed = lambda f: (seed(f) + 5003) % 10000              # noqa: E731  (the reference image uses other seeds than the runs)
    # warm-up: code objects, pool, rings
    r.reset_frame(); r.render_batch(1, [seed(1)] * K); r.render_adaptive(1, [seed(1)] * K, 0.05, min_frames=2); r.synchronize()

    t = time.perf_counter()
    r.reset_frame()
    for f in range(1, a.ref_frames + 1, 64):
        n = min(64, a.ref_frames + 1 - f)
        r.render_batch(f, [ref_seed(g) for g in range(f, f + n)])
    r.synchronize()
    t_ref = time.perf_counter() - t
    F = r.read_frame()
    with np.errstate(all="ignore"):
        ref_mean = (F[..., :3] / F[..., 3:4]).astype(np.float64)

    uni = []
    r.reset_frame()
    el = 0.0
    for f in range(1, a.frames + 1, K):
        t = time.perf_counter()
        r.render_batch(f, [seed(g) for g in range(f, f + K)])
        r.synchronize()
        dt = time.perf_counter() - t
        el += dt
        uni.append({"frames": f + K - 1, "s": round(el, 5), "msamples_s": round(W * H * K * spp / dt / 1e6, 1), "rmse": rmse(r.read_frame(), ref_mean)})
    ut = np.array([u["s"] for u in uni]); ue = np.array([u["rmse"] for u in uni])

    runs = []
    for rel in [float(x) for x in a.rel.split(",")]:
        r.reset_frame()
        calls, el, f = [], 0.0, 1
        while el < ut[-1] and f < 4096:
            t = time.perf_counter()
            n = r.render_adaptive(f, [seed(g) for g in range(f, f + K)], rel, 0.0, K, 0)
            r.synchronize()
            dt = time.perf_counter() - t
            el += dt
            F = r.read_frame()
            e = rmse(F, ref_mean)
            calls.append({"first_frame": f, "active_frac": round(n / (W * H), 5), "s": round(dt, 5), "elapsed_s": round(el, 5),
                          "msamples_s": round(n * K * spp / dt / 1e6, 1), "rmse": e,
                          "uniform_rmse_at_equal_time": float(np.interp(el, ut, ue)) if el >= ut[0] else None,
                          "mean_frames_per_pixel": round(float(F[..., 3].mean()), 3)})
            f += K
            if n == 0:
                break
        runs.append({"rel_err": rel, "calls": calls})
    r.close()
    out = {"scene": "C3", "W": W, "H": H, "spp_per_frame": spp, "chunk_frames": K, "reference": {"frames": a.ref_frames, "s": round(t_ref, 3)},
           "uniform": uni, "adaptive": runs}
    txt = json.dumps(out, indent=1)
    if a.out:
        open(a.out, "w").write(txt + "\n")
    print("uniform: frames  elapsed_s  Msamples/s  rmse")
    for u in uni:
        print(f"  {u['frames']:5d}  {u['s']:8.4f}  {u['msamples_s']:9.1f}  {u['rmse']:.5f}")
    for run in runs:
        print(f"adaptive rel_err={run['rel_err']}: frame  active  call_s  Msamples/s  elapsed_s  rmse  uniform_rmse@same_time")
        for c in run["calls"]:
            u = c["uniform_rmse_at_equal_time"]
            print(f"  {c['first_frame']:5d}  {c['active_frac']:.4f}  {c['s']:.4f}  {c['msamples_s']:9.1f}  {c['elapsed_s']:.4f}  {c['rmse']:.5f}  {'-' if u is None else f'{u:.5f}'}")


if __name__ == "__main__":
    main()
