#!/usr/bin/env python3
"""What the BVH refit (include/pt_refit.h) costs and what its trees are worth, against rebuilding the trees of the moved pose.

usage: refit_bench.py                 one child process per part: timing c4, timing big, quality m1, quality c4
       refit_bench.py timing c4|big   100 352 triangles (C4 with its mesh turned) | the 1 002 528-triangle mesh of scripts/big_scene.py (displaced)
       refit_bench.py quality m1|c4   steps 1-8: root_cost against the rest pose's, Msamples/s on the refit tree and on the rebuilt tree
       refit_bench.py probe c4|big    the plan, seven refits and three pt_build_bvh calls and nothing else, to run under a kernel trace

timing prints, from one run: pt_refit_create, pt_refit_run (best and median of 5), pt_build_bvh alone on the moved object's triangles, the CPU
rebuild (parse + build with the CPU builder less parse + build with the GPU builder plus pt_build_bvh alone, as scripts/bvh_bench.py has it), and
the whole step as a caller sees it, new binding 3 -> first rendered frame, by three routes: refit (move_triangles), rebuild (OBJ text of the
moved pose through the scene DSL with the GPU builder, pack, five uploads), and the uploads alone with a binding 10 that is already there (what
the host layout and the frame cost whoever computes the boxes).  Per-kernel times are not taken here: `probe` is the part to run under a kernel trace for those."""
import ctypes as C
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))


def _load():
    import ptimport
    pt = ptimport.load()
    from pathtracer_0_amd import hostlib, renderer, scenes
    return pt, hostlib, renderer, scenes


def c4_shell(scenes):
    """C4's scene (scenes.c4_mesh) before its one OBJ text is added"""
    sc = scenes._new_scene()
    scenes._cornell_materials(sc)
    sc.addMaterial("clay"); sc.setLastMtl("Kd", (0.7, 0.55, 0.4)); sc.setLastMtl("Pr", 1)
    return sc


def c4_text(scenes, step, nu=224, nv=224, seed=4):
    """C4's OBJ text with its mesh turned by 0.02 * step rad about the vertical through the room's centre"""
    o = scenes.Obj()
    scenes._cornell_room(o, boxes=False)
    o.group("torus"); o.usemtl("clay")
    v, n, f = scenes.displaced_torus(nu, nv, (0.0, 0.0, 0.0), 0.55, 0.22, 0.25, seed)
    a, b, t = 1.0, 0.4, 0.02 * step
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rt = np.array([[math.cos(t), 0, math.sin(t)], [0, 1, 0], [-math.sin(t), 0, math.cos(t)]])
    M = Rt @ Ry @ Rx
    P = np.asarray(v) @ M.T + np.array((0.0, 0.85, 0.1))
    N = np.asarray(n) @ M.T
    o.mesh([tuple(p) for p in P], [tuple(q) for q in N], f)
    return o.text()


def c4_pose(scenes, step, W, H, **kw):
    sc, text = c4_shell(scenes), c4_text(scenes, step, **kw)
    sc.addObjectText(text, 0, parentDirectory="")
    return scenes._finish("C4", sc, W, H, scenes.CORNELL_CAM, scenes.CORNELL_ROT, (0, 0, 0), 8, 8), text


def big_shell(hostlib):
    sc = hostlib.Scene()
    sc.addMaterial("ground"); sc.setLastMtl("Kd", (0.7, 0.6, 0.5)); sc.setLastMtl("Pr", 1)
    return sc


def big_text(step, qx=708, qy=708):
    """the mesh of scripts/big_scene.py under a ripple that grows with `step`: every vertex moves a little"""
    from bvh_bench import heightfield, obj_text
    v, f = heightfield(qx, qy)
    v = v.copy()
    v[:, 1] += 0.02 * step * np.sin(3.0 * v[:, 0] + 0.5 * step)
    return obj_text(v, f)


def big_pose(hostlib, scenes, step, W, H):
    sc, text = big_shell(hostlib), big_text(step)
    sc.use_gpu_bvh_builder(0)
    sc.addObjectText(text, 0)
    return scenes._finish("big", sc, W, H, (0.0, 0.8, -1.6), (0.35, 0.0, 0.0), (150, 180, 230), 4, 4), text


def tri9_of(tris, first):
    """pt_build_bvh's input for the triangles from `first` on: per triangle min, max, centroid in binary64"""
    t = np.asarray(tris, np.float32).reshape(-1, 40)[first:].astype(np.float64)
    v = np.stack([t[:, 0:3], t[:, 4:7], t[:, 8:11]], 1)
    return np.ascontiguousarray(np.concatenate([v.min(1), v.max(1), (v[:, 0] + (v[:, 1] + v[:, 2])) / 3.0], 1))


def timing(which, probe=False):
    pt, hostlib, renderer, scenes = _load()
    W, H = 640, 360
    hip = renderer.lib()
    hip.pt_build_bvh.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    warm = hostlib.Scene(); warm.addMaterial("m"); warm.use_gpu_bvh_builder(0)      # HIP runtime start-up outside the timings
    warm.addObjectText("o warm\nvn 0 1 0\nv 0 0 0\nv 1 0 0\nv 0 0 1\nv 1 0 1\nf 1//1 2//1 3//1\nf 2//1 4//1 3//1\n", 0)
    if which == "c4":
        scenes.GPU_BVH = 0
        rest, _ = c4_pose(scenes, 0, W, H)
        moved, text = c4_pose(scenes, 4, W, H)
        parts = lambda: c4_shell(scenes)                         # noqa: E731
        kw = dict(parentDirectory="")
    else:
        rest, _ = big_pose(hostlib, scenes, 0, W, H)
        moved, text = big_pose(hostlib, scenes, 4, W, H)
        parts = lambda: big_shell(hostlib)                       # noqa: E731
        kw = {}
    n = rest.buffers[3].size // 40
    assert moved.buffers[3].size == rest.buffers[3].size
    roots = rest.buffers[13]
    print(f"{which}: {n} triangles, {rest.buffers[11].size // 3} nodes, {int(roots[0])} roots", flush=True)

    t = time.perf_counter(); plan = renderer.RefitPlan(rest.buffers); t_create = time.perf_counter() - t
    _, rest_cost = plan.run(rest.buffers[3])
    runs = []
    for _ in range(5):
        t = time.perf_counter(); data, cost = plan.run(moved.buffers[3]); runs.append(time.perf_counter() - t)
    same_as_rest = bool(np.array_equal(plan.run(rest.buffers[3])[0].view(np.uint32), rest.buffers[10].view(np.uint32)))

    # pt_build_bvh alone on the moved object's triangles (the largest object: the last triangles of binding 3)
    mesh_first = n - (100352 if which == "c4" else n)
    tri9 = tri9_of(moved.buffers[3], mesh_first)
    m = len(tri9)
    nn, dep = C.c_int32(), C.c_int32()
    bounds = np.zeros((2 * m, 6)); links = np.zeros((2 * m, 2), np.int32); leaf = np.zeros((2 * m, 2), np.int32); order = np.zeros(m, np.int32)
    builds = []
    for _ in range(3):
        t = time.perf_counter()
        rc = hip.pt_build_bvh(0, tri9.ctypes.data, m, C.byref(nn), bounds.ctypes.data, links.ctypes.data, leaf.ctypes.data, order.ctypes.data, C.byref(dep))
        builds.append(time.perf_counter() - t)
        assert rc == 0
    if probe:
        plan.close()
        print(f"{which} probe: pt_refit_run best {min(runs) * 1e3:.2f} ms, pt_build_bvh alone best {min(builds) * 1e3:.2f} ms (under the tracer)", flush=True)
        return
    # the CPU rebuild, as scripts/bvh_bench.py derives it
    res = {}
    btext = text.encode()
    for name in ("cpu", "gpu"):
        sc = parts()
        sc.use_gpu_bvh_builder(0, enable=(name == "gpu"))
        t = time.perf_counter(); sc.addObjectText(btext, 0, **kw); res[name] = time.perf_counter() - t
    cpu_build = res["cpu"] - res["gpu"] + min(builds)
    print(f"{which}: pt_refit_create {t_create * 1e3:.2f} ms | pt_refit_run best {min(runs) * 1e3:.2f} ms, median {sorted(runs)[2] * 1e3:.2f} ms (5 runs; "
          f"{moved.buffers[3].nbytes / 1e6:.0f} MB up, {rest.buffers[10].nbytes / 1e6:.0f} MB down) | pt_build_bvh alone best {min(builds) * 1e3:.2f} ms, median "
          f"{sorted(builds)[1] * 1e3:.2f} ms ({m} triangles, {nn.value} nodes) | parse+build CPU {res['cpu']:.3f} s, GPU {res['gpu']:.3f} s => CPU rebuild ~{cpu_build:.3f} s | "
          f"refit of the rest pose gives back its binding 10: {same_as_rest} | root_cost moved / rest {cost.sum() / rest_cost.sum():.4f}", flush=True)

    # the whole step as a caller sees it: new binding 3 -> first rendered frame
    seeds = [scenes.frame_seed(f) for f in range(1, 8)]
    r = renderer.Renderer(W, H)
    r.load_workload(rest); r.reset_frame()
    r.render_batch(1, seeds[:1]); r.synchronize()
    t = time.perf_counter()
    r.move_triangles(plan, moved.buffers[3])
    t_move = time.perf_counter() - t
    r.reset_frame(); r.render_batch(1, seeds[1:2]); r.synchronize()
    t_refit_step = time.perf_counter() - t
    refit_frame = r.read_frame().copy()
    # the uploads alone (a binding 10 that is already there): the host layout and the frame
    r.load_workload(rest); r.reset_frame(); r.render_batch(1, seeds[:1]); r.synchronize()
    t = time.perf_counter()
    r.set_buffer(3, moved.buffers[3]); r.set_buffer(10, data)
    r.reset_frame(); r.render_batch(1, seeds[1:2]); r.synchronize()
    t_upload_step = time.perf_counter() - t
    # rebuild: the scene DSL with the GPU builder on the moved pose's OBJ text, pack, five uploads
    r.load_workload(rest); r.reset_frame(); r.render_batch(1, seeds[:1]); r.synchronize()
    t = time.perf_counter()
    sc = parts(); sc.use_gpu_bvh_builder(0); sc.addObjectText(btext, 0, **kw)
    bufs = sc.pack()
    t_built = time.perf_counter() - t
    for b in (3, 10, 11, 12, 13):
        r.set_buffer(b, bufs[b])
    r.reset_frame(); r.render_batch(1, seeds[1:2]); r.synchronize()
    t_rebuild_step = time.perf_counter() - t
    t = time.perf_counter(); r.reset_frame(); r.render_batch(1, seeds[2:3]); r.synchronize(); t_next = time.perf_counter() - t
    r.close(); plan.close()
    print(f"{which}: new binding 3 -> first frame ({W}x{H}): refit route {t_refit_step * 1e3:.1f} ms (of which move_triangles, the refit and two uploads, "
          f"{t_move * 1e3:.1f}) | uploads alone {t_upload_step * 1e3:.1f} ms | rebuild route {t_rebuild_step * 1e3:.1f} ms (of which parse + pt_build_bvh + pack "
          f"{t_built * 1e3:.1f}) | a frame with nothing uploaded {t_next * 1e3:.1f} ms | refit frame finite: {bool(np.isfinite(refit_frame[..., 3]).all())}", flush=True)


def quality(which):
    pt, hostlib, renderer, scenes = _load()
    scenes.GPU_BVH = 0
    W, H, frames = (96 * 4, 54 * 4, 8) if which == "m1" else (640, 360, 8)
    pose = (lambda s: scenes.m1_moving(s, W, H)) if which == "m1" else (lambda s: c4_pose(scenes, s, W, H)[0])
    rest = pose(0)
    plan = renderer.RefitPlan(rest.buffers)
    _, rest_cost = plan.run(rest.buffers[3])
    seeds = [scenes.frame_seed(f) for f in range(1, frames + 1)]
    r = renderer.Renderer(W, H)
    r.load_workload(rest)

    def rate():
        best = 0.0
        for _ in range(3):
            r.reset_frame(); r.synchronize()
            t = time.perf_counter(); r.render_batch(1, seeds); r.synchronize(); dt = time.perf_counter() - t
            best = max(best, W * H * rest.sample_res * frames / dt / 1e6)
        return best

    rate()                                                          # warm-up: kernels loaded, pool sized
    print(f"{which} {W}x{H}, {frames} frames x {rest.sample_res} spp, best of 3: rest pose {rate():.1f} Msamples/s", flush=True)
    for step in range(1, 9):
        wl = pose(step)
        for b in (3, 7, 10, 11, 12, 13):
            r.set_buffer(b, wl.buffers[b])
        rebuilt = rate()
        for b in (11, 12, 13):
            r.set_buffer(b, rest.buffers[b])
        _, cost = r.move_triangles(plan, wl.buffers[3])
        refit = rate()
        same_topology = all(np.array_equal(wl.buffers[b], rest.buffers[b]) for b in (11, 12, 13))
        print(f"{which} step {step}: root_cost / rest {cost.sum() / rest_cost.sum():.4f} | refit tree {refit:.1f} Msamples/s, rebuilt tree {rebuilt:.1f} "
              f"({refit / rebuilt:.3f}) | rebuilt topology equals the rest pose's: {same_topology}", flush=True)
    r.close(); plan.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "probe":
        timing(sys.argv[2], probe=True)
    elif len(sys.argv) == 3 and sys.argv[1] in ("timing", "quality"):
        (timing if sys.argv[1] == "timing" else quality)(sys.argv[2])
    else:
        for part in (("timing", "c4"), ("timing", "big"), ("quality", "m1"), ("quality", "c4")):
            rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(part), timeout=900).returncode
            if rc != 0:
                sys.exit(f"refit_bench.py {' '.join(part)} ended with {rc}: nothing further is started")
