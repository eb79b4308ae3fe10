#!/usr/bin/env python3
"""Quality and cost of the reprojection across moved geometry with bilinear taps (include/pt_motion_bilinear.h) -> profiles/r20_motion_bilinear.txt.

usage: motion_bilinear_quality.py [--out FILE] [--ref-frames N]   the quality walk and the wall times, appended to FILE
       motion_bilinear_quality.py --probe                         the three calls with no rendering: run under a kernel-trace statistics pass of its own

Walk: M1 at 1920 x 1080 under a fixed camera, with and without its texture (albedo_floor 0.05 / 0), poses m1_moving(0.25 * i): K frames in the rest
pose, then STEPS steps of (mark, upload the next pose, carry, K frames) with pt_reproject_frame_moved and with pt_reproject_frame_moved_bilinear on the
same seeds, and a reset with K frames of the last pose: the kept fractions per step and, at the last step, the clamped RMSE of the means against a
reference of the last pose (seeds of its own), over the image and over the pixels on a moved primitive then or now.
Wall: three calls each of the two moved calls on the same image, mark and move, after a first call that takes the allocations."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1920, 1080
STEPS = 16
STEP = 0.25
K = 4
GEOMETRY = (3, 7, 10, 11, 12, 13)
SCENES = ((False, 0.0), (True, 0.05))
SHIFT = np.array([0.011, 0.0, 0.017], np.float32)


def upload(r, wl):
    for b in GEOMETRY:
        r.set_buffer(b, wl.buffers[b])


def mean_of(f):
    return f[..., :3].astype(np.float64) / np.maximum(f[..., 3:4].astype(np.float64), 1e-30)


def clamped_rmse(a, b, where):
    d = np.clip(a, 0, 1) - np.clip(b, 0, 1)
    ok = where & np.isfinite(d).all(-1)
    return float(np.sqrt((d[ok] ** 2).mean()))


def carry(r, how, floor):
    """(kept, blended, wall seconds)"""
    t0 = time.perf_counter()
    if how == "bilinear":
        kept, blended = r.reproject_frame_moved_bilinear(albedo_floor=floor)
    else:
        kept, blended = r.reproject_frame_moved(albedo_floor=floor), 0
    return kept, blended, time.perf_counter() - t0


def walk(r, poses, seed, how, floor):
    """FRAME after the last step and per step (kept, blended) as fractions; how = nearest, bilinear or reset"""
    upload(r, poses[0])
    r.reset_frame()
    frame, out = 1, []
    r.render_batch(frame, [seed(frame + f) for f in range(K)])
    frame += K
    for wl in poses[1:]:
        if how == "reset":
            upload(r, wl)
            r.reset_frame()
            out.append((0.0, 0.0))
        else:
            r.motion_mark()
            upload(r, wl)
            kept, blended, _ = carry(r, how, floor)
            out.append((kept / (W * H), blended / (W * H)))
        r.render_batch(frame, [seed(frame + f) for f in range(K)])
        frame += K
    r.synchronize()
    return r.read_frame(), out


def on_moved(r, wl_then, wl_now):
    """the pixels on a moved primitive, then or now, from the device's own records of the two poses"""
    import _motion_model as MM
    upload(r, wl_then)
    rh = r.read_features()
    upload(r, wl_now)
    rn = r.read_features()
    geo = (MM.tri_vertices(wl_now.buffers[3]), MM.tri_vertices(wl_then.buffers[3]), MM.ellipsoids(wl_now.buffers[7]), MM.ellipsoids(wl_then.buffers[7]))
    org = np.asarray(wl_now.buffers[0], np.float32)[:3]
    kn = MM.moved_point(rn, org, *geo)[3].reshape(H, W)
    kh = MM.moved_point(rh, org, geo[1], geo[0], geo[3], geo[2])[3].reshape(H, W)
    return (kn >= 2) | (kh >= 2)


def image(seed=3):
    rs = np.random.RandomState(seed)
    cnt = rs.randint(1, 100, size=(H, W, 1)).astype(np.float32)
    fr = np.concatenate([rs.rand(H, W, 3).astype(np.float32) * cnt, cnt], -1)
    n = rs.randint(1, 100, size=(H, W)).astype(np.float32)
    Y = rs.rand(H, W).astype(np.float32)
    return fr, np.stack([n * Y, n * Y * Y * 1.25, n, np.zeros_like(n)], -1).astype(np.float32)


def prepared(r, wl0, wl1, fr, T, moved_camera):
    """FRAME and T under pose 0 and its camera, marked, pose 1 uploaded (and the camera moved)"""
    upload(r, wl0)
    r.set_buffer(0, wl0.buffers[0])
    r.write_frame(fr)
    r.write_moments(T)
    r.motion_mark()
    upload(r, wl1)
    if moved_camera:
        o = np.asarray(wl0.buffers[0], np.float32).copy()
        o[:3] += SHIFT
        r.set_buffer(0, o)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--ref-frames", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_motion_bilinear.txt"))
    a = ap.parse_args()
    import ptimport
    pt = ptimport.load()
    from pathtracer_0_amd import renderer
    seed = pt.scenes.frame_seed
    L = []
    wl0, wl1 = pt.scenes.m1_moving(0, W, H), pt.scenes.m1_moving(STEP, W, H)
    fr, T = image()
    if a.probe:
        # each kernel five times per floor: the moved call (k_reproject<true, ., false>), the bilinear call under a moved camera in the moved scene
        # (k_reproject<false, ., true>) and the moved bilinear call (k_reproject<true, ., true>), all on the same image
        r = renderer.Renderer(W, H)
        r.load_workload(wl0)
        for i in range(5):
            for floor in (0.0, 0.05):
                prepared(r, wl0, wl1, fr, T, True)
                print(f"moved nearest floor {floor}: kept %d blended %d wall %.2f ms" % tuple(x * (1e3 if j == 2 else 1) for j, x in enumerate(carry(r, "nearest", floor))))
                prepared(r, wl0, wl1, fr, T, True)
                print(f"moved bilinear floor {floor}: kept %d blended %d wall %.2f ms" % tuple(x * (1e3 if j == 2 else 1) for j, x in enumerate(carry(r, "bilinear", floor))))
                upload(r, wl1)
                r.set_buffer(0, wl0.buffers[0])
                r.write_frame(fr)
                r.write_moments(T)
                o = np.asarray(wl0.buffers[0], np.float32).copy()
                o[:3] += SHIFT
                r.set_buffer(0, o)
                t0 = time.perf_counter()
                kept, blended = r.reproject_frame_bilinear(albedo_floor=floor)
                print(f"camera bilinear floor {floor}: kept {kept} blended {blended} wall {1e3 * (time.perf_counter() - t0):.2f} ms")
        r.close()
        print("probe done")
        return
    L.append(f"wall time of the call, M1 textured {W}x{H}, pose 0 -> {STEP}, fixed camera, T allocated, three calls each after one that takes the allocations; "
             f"scripts/motion_bilinear_quality.py")
    r = renderer.Renderer(W, H)
    r.load_workload(wl0)
    for floor in (0.0, 0.05):
        times = {}
        for how in ("nearest", "bilinear"):
            ts = []
            for i in range(4):
                prepared(r, wl0, wl1, fr, T, False)
                kept, blended, t = carry(r, how, floor)
                ts.append(1e3 * t)
            times[how] = (ts[1:], kept, blended)
        n, b = times["nearest"], times["bilinear"]
        L.append(f"  albedo_floor {floor}: pt_reproject_frame_moved " + " / ".join(f"{t:.2f}" for t in n[0]) + f" ms (kept {n[1]}); pt_reproject_frame_moved_bilinear "
                 + " / ".join(f"{t:.2f}" for t in b[0]) + f" ms (kept {b[1]}, blended {b[2]}); medians differ by {np.median(b[0]) - np.median(n[0]):+.2f} ms, "
                 f"spread {max(n[0]) - min(n[0]):.2f} / {max(b[0]) - min(b[0]):.2f} ms")
    r.close()
    L.append(f"quality walk, M1 {W}x{H}, fixed camera, {STEPS} steps of {STEP} of m1_moving, {K} frames per step, rule (64, 0.02, 0.9), snap 1/64; clamped RMSE of the "
             f"means at the last step against {a.ref_frames} frames of the last pose with seeds of their own")
    for textured, floor in SCENES:
        poses = [pt.scenes.m1_moving(STEP * i, W, H, textured=textured) for i in range(STEPS + 1)]
        r = renderer.Renderer(W, H)
        r.load_workload(poses[0])
        r.record_moments(True)
        upload(r, poses[-1])
        r.reset_frame()
        for f0 in range(1, a.ref_frames + 1, 64):
            n = min(64, a.ref_frames + 1 - f0)
            r.render_batch(f0, [seed(5000 + f) for f in range(f0, f0 + n)])
        ref = mean_of(r.read_frame())
        moved = on_moved(r, poses[-2], poses[-1])
        every = np.ones((H, W), bool)
        L.append(f"  M1 {'textured' if textured else 'untextured'}, albedo_floor {floor}, T recorded; pixels on a moved primitive, then or now, at the last step: {int(moved.sum())}")
        for how in ("nearest", "bilinear", "reset"):
            frame, fracs = walk(r, poses, seed, how, floor)
            m = mean_of(frame)
            line = f"    {how:8s} clamped RMSE whole image {clamped_rmse(m, ref, every):.5f}, on moved primitives {clamped_rmse(m, ref, moved):.5f}"
            if how != "reset":
                line += (f"; kept per step {min(x[0] for x in fracs):.5f} .. {max(x[0] for x in fracs):.5f}"
                         + (f", blended {min(x[1] for x in fracs):.5f} .. {max(x[1] for x in fracs):.5f}" if how == "bilinear" else ""))
            L.append(line)
        r.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
