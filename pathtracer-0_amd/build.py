"""Build recipes for the native libraries (in-tree, so the .so files travel with the snapshot).

  libpt_host.so  g++    host-side scene producers (csrc/host/scene_host.cpp)
  libpt_hip.so   hipcc  gfx950 render path + C ABI (csrc/hip/pt_hip.hip), GPU BVH builder (csrc/hip/pt_bvh.hip),
                 a-trous denoiser (csrc/hip/pt_denoise.hip), reprojection (csrc/hip/pt_reproject.hip), variance-guided filter and its selection (csrc/hip/pt_guided.hip),
                 each of the last two with its albedo-demodulated form (include/pt_demod.h); the prefill of unrendered pixels (include/pt_fill.h) in pt_guided.hip;
                 the seen-through feature records (include/pt_through.h) in pt_hip.hip; the reprojection across moved geometry (include/pt_motion.h) and
                 the history validation (include/pt_validate.h) and the reprojection through mirror and glass chains (include/pt_reproject_through.h) and with bilinear taps (include/pt_reproject_bilinear.h; across moved geometry: include/pt_motion_bilinear.h) in pt_reproject.hip.  pt_denoise.hip, pt_reproject.hip and pt_guided.hip are called through csrc/hip/pt_image_launch.hpp by the host half of the image-space passes,
                 csrc/hip/pt_image.hpp (included by pt_hip.hip).  The scene build is two halves: csrc/hip/pt_scene_layout.hpp validates the buffers and lays out
                 the record arrays of csrc/hip/pt_scene_records.hpp on the host (no HIP call: tests/c/scene_layout_check.cpp compiles it with g++), buildScene in
                 pt_hip.hip uploads them.  csrc/hip/pt_launch_plan.hpp plans every intersect launch and the pool's and the ring's sizes, host only as well
                 (tests/c/launch_plan_check.cpp), csrc/hip/pt_stream_sched.hpp schedules the frame stream (tests/c/stream_sched_check.cpp), and
                 csrc/hip/pt_image_history.hpp keeps what the current image is a picture of: camera records, upload generations, the validity of the
                 mark and the hold, the record caches' keys (tests/c/image_history_check.cpp).  csrc/hip/pt_options.hpp holds the tuning options of
                 pt_set_option: the struct the layout step and the planner read, and the one table that defines each option (tests/c/options_check.cpp).
                 csrc/hip/pt_image_args.hpp holds what every image-space call refuses in its arguments, one row per entry point, and
                 csrc/hip/pt_motion_pack.hpp packs the primitives' positions for the reprojection across moved geometry (tests/c/image_args_check.cpp).
                 The refit of a scene's BVHs to moved triangles (include/pt_refit.h) is csrc/hip/pt_refit.hip, a scene-build kernel like pt_bvh.hip, behind
                 its host-only planning step csrc/hip/pt_refit_plan.hpp (tests/c/refit_plan_check.cpp); csrc/hip/pt_refit_state.hpp is what a plan holds.
                 The in-place move of a scene's triangles (include/pt_move.h) patches the device records after a refit: csrc/hip/pt_move.hip, a scene-build
                 kernel file as well, behind csrc/hip/pt_move_launch.hpp; its host-only step csrc/hip/pt_scene_move.hpp (the map of the record order and
                 the CPU statement of the patch, tests/c/scene_move_check.cpp) and its host half csrc/hip/pt_move_host.hpp (included by pt_image.hpp).
                 The outlier rejection (include/pt_despeckle.h) is csrc/hip/pt_despeckle.hip, an image-space kernel file like pt_reproject.hip, behind
                 csrc/hip/pt_image_launch.hpp; its host-only argument check csrc/hip/pt_despeckle_rule.hpp (tests/c/despeckle_rule_check.cpp) and its
                 host half csrc/hip/pt_despeckle_host.hpp (included by pt_image.hpp).
                 The display image (include/pt_tonemap.h: metered exposure, tone curve, sRGB transfer) is csrc/hip/pt_tonemap.hip, an image-space
                 kernel file as well, behind csrc/hip/pt_image_launch.hpp; its host-only step csrc/hip/pt_tonemap_rule.hpp (the argument check, the
                 metered exposure and the sRGB threshold table that scripts/tonemap_srgb_table.py generates; tests/c/tonemap_rule_check.cpp) and
                 its host half csrc/hip/pt_tonemap_host.hpp (included by pt_image.hpp)
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
# numeric contract: no implicit FMA contraction, IEEE divide/sqrt
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fPIC", "-shared",
             "-Wall", "-Wno-unused-value"]
HOST_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra"]


def _stale(out, srcs):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(s) > t for s in srcs)


def build_host(force=False):
    src = os.path.join(HERE, "csrc", "host", "scene_host.cpp")
    hdr = os.path.join(HERE, "..", "include", "pt_scene.h")
    out = os.path.join(HERE, "libpt_host.so")
    if force or _stale(out, [src, hdr]):
        subprocess.check_call(["g++"] + HOST_FLAGS + ["-o", out, src])
    return out


LLVM_BIN = "/opt/rocm/lib/llvm/bin"


def assemble_extend(out_inc=None, defines=()):
    """pt_extend_gfx950.s (the hand-written intersect kernel) -> eighteen code objects (16- / 18- / 24-bit traversal-stack entries x numeric contract x block size) -> a header of
    byte arrays that pt_hip.hip embeds and loads with hipModuleLoadData.  The header is generated, never committed."""
    d = os.path.join(HERE, "csrc", "hip")
    src = os.path.join(d, "pt_extend_gfx950.s")
    out_inc = out_inc or os.path.join(d, "pt_extend_hsaco.inc")
    tmp = os.path.join(HERE, "..", "build", "asm", os.path.splitext(os.path.basename(out_inc))[0])      # per target: variants build in parallel
    os.makedirs(tmp, exist_ok=True)
    text = ["// generated by build.py from pt_extend_gfx950.s - do not edit\n"]
    # f: the relaxed numeric contract (v_rcp_f32 for 1/d and 1/det); w: 1024-thread blocks (a context alone on its GPU: 2 blocks per CU share a 32 KB tile)
    # (h: 512-thread blocks, an option of pt_set_option 17: 3 blocks per CU over a 32 KB tile when streams share the GPU)
    # p24: 24-bit entries — 16 bits in the LDS stacks, 8 in a second LDS array of bytes (trees beyond 131071 nodes: the meshes of millions of triangles)
    variants = [(n + w, p, f, t) for w, t in (("", 8), ("w", 10), ("h", 9)) for n, p, f in (("s16", 0, 0), ("p18", 1, 0), ("s16f", 0, 1), ("p18f", 1, 1), ("p24", 2, 0), ("p24f", 2, 1))]
    for name, packed, fast, log_tpb in variants:
        obj, co = os.path.join(tmp, f"pt_extend_{name}.o"), os.path.join(tmp, f"pt_extend_{name}.hsaco")
        subprocess.check_call([os.path.join(LLVM_BIN, "clang"), "-x", "assembler-with-cpp", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950",
                               f"-DPACKED18={1 if packed == 1 else 0}", f"-DPACKED24={1 if packed == 2 else 0}", f"-DFAST_RCP={fast}", f"-DLOG_TPB={log_tpb}"] + list(defines) + ["-c", src, "-o", obj])
        subprocess.check_call([os.path.join(LLVM_BIN, "ld.lld"), "-shared", obj, "-o", co])
        data = open(co, "rb").read()
        text.append(f"alignas(4096) static const unsigned char pt_extend_hsaco_{name}[{len(data)}] = {{\n")
        text += [",".join(str(b) for b in data[i:i + 64]) + ",\n" for i in range(0, len(data), 64)]
        text.append("};\n")
    new = "".join(text)
    if not os.path.exists(out_inc) or open(out_inc).read() != new:
        open(out_inc, "w").write(new)
    return out_inc


def build_hip(force=False, extra=(), asm_defines=()):
    d = os.path.join(HERE, "csrc", "hip")
    srcs = [os.path.join(d, f) for f in ("pt_hip.hip", "pt_bvh.hip", "pt_denoise.hip", "pt_reproject.hip", "pt_guided.hip", "pt_refit.hip", "pt_move.hip", "pt_despeckle.hip", "pt_tonemap.hip", "pt_device.hpp", "pt_math.hpp", "pt_multi.hpp", "pt_image.hpp", "pt_image_launch.hpp", "pt_devmem.hpp", "pt_scene_records.hpp", "pt_scene_layout.hpp", "pt_options.hpp", "pt_launch_plan.hpp", "pt_stream_sched.hpp", "pt_image_history.hpp", "pt_image_args.hpp", "pt_motion_pack.hpp", "pt_refit_plan.hpp", "pt_refit_state.hpp", "pt_scene_move.hpp", "pt_move_host.hpp", "pt_move_launch.hpp", "pt_despeckle_rule.hpp", "pt_despeckle_host.hpp", "pt_tonemap_rule.hpp", "pt_tonemap_host.hpp", "pt_extend_gfx950.s")] + [os.path.join(HERE, "..", "include", h) for h in ("pt_api.h", "pt_debug.h", "pt_adaptive.h", "pt_denoise.h", "pt_reproject.h", "pt_guided.h", "pt_steer.h", "pt_demod.h", "pt_fill.h", "pt_through.h", "pt_motion.h", "pt_validate.h", "pt_reproject_through.h", "pt_reproject_bilinear.h", "pt_motion_bilinear.h", "pt_refit.h", "pt_move.h", "pt_despeckle.h", "pt_tonemap.h")]
    out = os.path.join(HERE, "libpt_hip.so")
    if force or _stale(out, srcs):
        assemble_extend(defines=asm_defines)
        hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
        subprocess.check_call([hipcc] + HIP_FLAGS + list(extra) + ["-o", out] + srcs[:9])
    return out


def kernel_source_hash():
    """sha256 (16 hex digits) over the sources of the render kernels, in name order: committed counter summaries (profiles/pmc_*.json) carry it,
    and bench.py flags them stale when the kernels have changed underneath.  (pt_multi.hpp — host-side orchestration of several streams —, pt_image.hpp and
    pt_image_launch.hpp — the host half and the launch interface of the image-space passes —, pt_scene_layout.hpp — the host-only layout step of the
    scene build; the records it fills, which the kernels read, are pt_scene_records.hpp and part of it —, pt_launch_plan.hpp — the host-only planning
    of the intersect launches —, pt_stream_sched.hpp and pt_image_history.hpp — the host-only scheduler and image bookkeeping —, pt_options.hpp — the option table —, pt_image_args.hpp and pt_motion_pack.hpp — the argument table of the image-space calls and the motion packing —, pt_despeckle.hip with pt_despeckle_rule.hpp and pt_despeckle_host.hpp, and pt_tonemap.hip with pt_tonemap_rule.hpp and pt_tonemap_host.hpp — image-space passes, as pt_reproject.hip is — and pt_bvh.hip, pt_refit.hip with pt_refit_plan.hpp and pt_refit_state.hpp, and pt_move.hip with pt_scene_move.hpp, pt_move_host.hpp and
    pt_move_launch.hpp — the scene-build kernels — are not part of it.)"""
    import hashlib
    d = os.path.join(HERE, "csrc", "hip")
    h = hashlib.sha256()
    for f in ("pt_device.hpp", "pt_extend_gfx950.s", "pt_hip.hip", "pt_math.hpp", "pt_scene_records.hpp"):
        h.update(f.encode()); h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def build_all(force=False):
    return build_host(force), build_hip(force)


if __name__ == "__main__":
    print(build_all(force=True))
