"""Render call of the reference behind the C ABI (include/pt_api.h), Python face.

`Renderer` plays the part of the GL state the reference's frame loop drives
(/root/reference/src/Main/dispatch.java:590-713): set_buffer == glBufferData/glBufferSubData on
an SSBO binding point, set_texture == texture upload, reset_frame == resetTexture (:732-735),
render(frame_count, seed) == glUniform1i x2 + glDrawArrays (:697-705), read_frame == glReadPixels
of the RGBA32F accumulation image.  There is no CPU fallback: constructing a Renderer without
the HIP library or without a gfx950 device raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

COUNTERS = ["segments", "nodes", "tritests", "hitupd", "samples", "boxtests", "iterations", "extend_launches"]
KERNELS = {"extend": 0, "shade": 1, "generate": 2, "accumulate": 3}
OPTIONS = {"path_slots": 0, "count_stats": 1, "lds_budget": 2, "none_min": 3, "extend_mode": 4, "extend_tpb": 5, "extend_cache_bytes": 6,
           "refill_min": 7, "extend_blocks_per_cu": 8, "inner_keep_eighths": 9, "bfs_nodes": 10, "stack_mode": 11,
           "query_asm_eligible": 12, "query_asm_launches_above": 13, "asm_loop": 14, "numeric_contract": 16, "asm_tpb": 17, "index_stack_8bit": 18, "asm_node_layout": 19, "asm_root_cull": 20, "cu_partition": 21}

# the device record arrays pt_debug_scene_records reads back (include/pt_debug.h), with the element type each comes back as
SCENE_RECORDS = {"nodes": (0, np.float32), "nodes80": (1, np.float32), "tris": (2, np.float32), "shade": (3, np.float32), "roots": (4, np.float32),
                 "ellip": (5, np.float32), "triObj": (6, np.int32)}

# the albedo_floor to pass for the demodulated calls of include/pt_demod.h (albedo_floor=ALBEDO_FLOOR; the keyword's own default None makes the
# plain call): scripts/demod_quality.py's grid on T1, C3 and C6 (profiles/r13_demod_quality.txt)
ALBEDO_FLOOR = 0.2


def hip_runtimes_mapped():
    """real paths of every libamdhip64 mapped into this process (Linux)"""
    out = set()
    try:
        for line in open("/proc/self/maps"):
            p = line.rstrip("\n").split(" ")[-1]
            if "libamdhip64" in os.path.basename(p):
                out.add(os.path.realpath(p))
    except OSError:
        pass
    return sorted(out)


def hip_runtime_info():
    """{"path", "version"} of the HIP runtime this process runs on (hipRuntimeGetVersion of the mapped libamdhip64)"""
    rts = hip_runtimes_mapped()
    if not rts:
        return {"path": None, "version": None}
    v = C.c_int(0)
    try:
        C.CDLL(rts[0]).hipRuntimeGetVersion(C.byref(v))
    except (OSError, AttributeError):
        pass
    return {"path": rts[0], "version": v.value, "runtimes_mapped": len(rts)}


def _load_one_hip_runtime(path):
    """libpt_hip.so is linked against libamdhip64.so.7 (RUNPATH: the ROCm installation it was built with).  PyTorch ships its OWN
    libamdhip64.so with the same SONAME.  A process must run on ONE of them:
      * torch imported first  -> the dynamic loader resolves the library's libamdhip64.so.7 to torch's copy, already mapped: one runtime;
      * library loaded first  -> ROCm's runtime is mapped and initialises the GPU; a later `import torch` maps a SECOND runtime, which finds
        no device ("No HIP GPUs are available", profiles/r03_a_hip_runtime_probe.txt — the failure conftest.py used to paper over).
    So: a Python host that will also use torch (bench.py, the tests, shard.py) gets torch imported here, before the library; a process that
    ends up with two runtimes mapped is refused.  PT_NO_TORCH=1: never import torch (a torch-free host; it then runs on ROCm's runtime)."""
    import sys
    if "torch" not in sys.modules and os.environ.get("PT_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401  (maps torch's HIP runtime first)
        except ImportError:
            pass
    L = C.CDLL(path)
    rts = hip_runtimes_mapped()
    if len(rts) > 1 and os.environ.get("PT_ALLOW_TWO_HIP_RUNTIMES") != "1":
        raise RuntimeError("two HIP runtimes are mapped into this process: " + ", ".join(rts) + ".  libpt_hip.so and PyTorch must share one: "
                           "import torch BEFORE the first pathtracer_0_amd.renderer call (or set PT_NO_TORCH=1 and do not import torch at all)")
    return L


def lib():
    global _LIB
    if _LIB is None:
        path = os.environ.get("PT_HIP_LIB") or os.path.join(_HERE, "libpt_hip.so")     # PT_HIP_LIB: A/B builds of the same ABI (tuning only)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: the HIP extension is required (no fallback). Build it with __graft_entry__.build()")
        L = _load_one_hip_runtime(path)
        vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
        L.pt_last_error.restype = C.c_char_p
        L.pt_create.argtypes = [C.POINTER(vp), ci, ci, ci, ci, ci]
        L.pt_create_multi.argtypes = [C.POINTER(vp), C.POINTER(ci), ci, ci, ci]
        L.pt_create_multi_part.argtypes = [C.POINTER(vp), C.POINTER(ci), ci, ci, ci, ci, ci]
        L.pt_gather_image.argtypes = [vp, ci, C.POINTER(vp)]
        L.pt_destroy.argtypes = [vp]
        L.pt_set_buffer.argtypes = [vp, ci, vp, sz]
        L.pt_set_texture.argtypes = [vp, ci, ci, ci, vp]
        L.pt_reset_frame.argtypes = [vp]
        L.pt_render.argtypes = [vp, ci, ci]
        L.pt_render_batch.argtypes = [vp, ci, ci, vp]
        L.pt_render_batch_async.argtypes = [vp, ci, ci, vp]
        L.pt_next_image.argtypes = [vp]
        L.pt_finish_image.argtypes = [vp, ci]
        L.pt_image_device.argtypes = [vp, ci, C.POINTER(vp), C.POINTER(sz)]
        L.pt_synchronize.argtypes = [vp]
        L.pt_stream_wait.argtypes = [vp]
        L.pt_read_frame.argtypes = [vp, vp]
        if hasattr(L, "pt_write_frame"):                      # (absent in A/B builds of earlier rounds loaded through PT_HIP_LIB)
            L.pt_write_frame.argtypes = [vp, vp]
        L.pt_read_display.argtypes = [vp, ci, ci, vp]
        L.pt_save_png.argtypes = [vp, ci, ci, C.c_char_p]
        L.pt_frame_device.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
        L.pt_shard_slots.argtypes = [ci, ci, ci, C.POINTER(sz)]
        L.pt_shard_map.argtypes = [ci, ci, ci, ci, vp, sz]
        L.pt_unshard.argtypes = [vp, vp, vp]
        L.pt_set_stream.argtypes = [vp, vp]
        L.pt_set_option.argtypes = [vp, ci, C.c_int64]
        L.pt_get_counters.argtypes = [vp, vp, ci]
        L.pt_reset_counters.argtypes = [vp]
        L.pt_kernel_time.argtypes = [vp, ci, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        L.pt_set_timing.argtypes = [vp, ci]
        L.pt_kernel_time_median.argtypes = [vp, ci, C.POINTER(C.c_double)]
        L.pt_debug_math.argtypes = [vp, ci, vp, vp, vp, sz]
        L.pt_debug_intersect.argtypes = [vp, vp, vp, vp, sz]
        if hasattr(L, "pt_render_adaptive"):                  # include/pt_adaptive.h
            L.pt_render_adaptive.argtypes = [vp, ci, ci, vp, C.c_float, C.c_float, ci, ci, C.POINTER(C.c_int64)]
            L.pt_read_display_mean.argtypes = [vp, ci, vp]
        if hasattr(L, "pt_denoise"):                          # include/pt_denoise.h
            cf = C.c_float
            L.pt_read_features.argtypes = [vp, vp]
            L.pt_denoise.argtypes = [vp, ci, cf, cf, cf, cf, vp]
            L.pt_read_display_denoised.argtypes = [vp, ci, cf, cf, cf, cf, ci, vp]
        if hasattr(L, "pt_reproject_frame"):                  # include/pt_reproject.h
            L.pt_reproject_frame.argtypes = [vp, C.c_float, C.c_float, C.c_float, ci, C.POINTER(C.c_int64)]
        if hasattr(L, "pt_denoise_guided"):                   # include/pt_guided.h
            cf = C.c_float
            L.pt_record_moments.argtypes = [vp, ci]
            L.pt_read_moments.argtypes = [vp, vp]
            L.pt_write_moments.argtypes = [vp, vp]
            L.pt_denoise_guided.argtypes = [vp, ci, cf, cf, cf, cf, ci, vp]
            L.pt_read_display_denoised_guided.argtypes = [vp, ci, cf, cf, cf, cf, ci, ci, vp]
        if hasattr(L, "pt_render_mask"):                      # include/pt_steer.h
            L.pt_render_mask.argtypes = [vp, ci, ci, vp, vp, C.POINTER(C.c_int64)]
            L.pt_select_guided.argtypes = [vp, C.POINTER(GuidedRule), vp, C.POINTER(C.c_int64)]
            L.pt_render_adaptive_guided.argtypes = [vp, ci, ci, vp, C.POINTER(GuidedRule), C.POINTER(C.c_int64)]
        if hasattr(L, "pt_denoise_guided_demod"):             # include/pt_demod.h
            cf = C.c_float
            L.pt_denoise_guided_demod.argtypes = [vp, ci, cf, cf, cf, cf, ci, cf, vp]
            L.pt_read_display_denoised_guided_demod.argtypes = [vp, ci, cf, cf, cf, cf, ci, cf, ci, vp]
            L.pt_select_guided_demod.argtypes = [vp, C.POINTER(GuidedRule), cf, vp, C.POINTER(C.c_int64)]
            L.pt_render_adaptive_guided_demod.argtypes = [vp, ci, ci, vp, C.POINTER(GuidedRule), cf, C.POINTER(C.c_int64)]
            L.pt_reproject_frame_demod.argtypes = [vp, cf, cf, cf, ci, cf, C.POINTER(C.c_int64)]
        if hasattr(L, "pt_fill_frame"):                       # include/pt_fill.h
            cf = C.c_float
            L.pt_render_interleaved.argtypes = [vp, ci, ci, vp, ci, ci, ci, C.POINTER(C.c_int64)]
            L.pt_fill_frame.argtypes = [vp, cf, cf, cf, cf, vp, C.POINTER(C.c_int64)]
            L.pt_denoise_guided_filled.argtypes = [vp, ci, cf, cf, cf, cf, ci, cf, vp]
            L.pt_read_display_denoised_guided_filled.argtypes = [vp, ci, cf, cf, cf, cf, ci, cf, ci, vp]
        if hasattr(L, "pt_read_features_through"):            # include/pt_through.h
            cf = C.c_float
            tr = C.POINTER(ThroughRule)
            L.pt_read_features_through.argtypes = [vp, tr, vp]
            L.pt_read_through_rays.argtypes = [vp, tr, vp]
            L.pt_fill_frame_through.argtypes = [vp, tr, cf, cf, cf, cf, vp, C.POINTER(C.c_int64)]
            L.pt_denoise_guided_through.argtypes = [vp, tr, ci, cf, cf, cf, cf, ci, cf, vp]
            L.pt_read_display_denoised_guided_through.argtypes = [vp, tr, ci, cf, cf, cf, cf, ci, cf, ci, vp]
        if hasattr(L, "pt_motion_mark"):                      # include/pt_motion.h
            cf = C.c_float
            L.pt_motion_mark.argtypes = [vp]
            L.pt_reproject_frame_moved.argtypes = [vp, cf, cf, cf, ci, cf, C.POINTER(C.c_int64)]
        if hasattr(L, "pt_history_hold"):                     # include/pt_validate.h
            L.pt_history_hold.argtypes = [vp]
            L.pt_history_merge.argtypes = [vp, C.POINTER(ValidateRule), vp, C.POINTER(C.c_int64)]
        if hasattr(L, "pt_despeckle"):                        # include/pt_despeckle.h
            L.pt_despeckle.argtypes = [vp, C.POINTER(DespeckleRule), vp, vp, C.POINTER(C.c_int64)]
            L.pt_despeckle_frame.argtypes = [vp, C.POINTER(DespeckleRule), vp, C.POINTER(C.c_int64)]
        if hasattr(L, "pt_tonemap"):                          # include/pt_tonemap.h
            L.pt_tonemap.argtypes = [vp, C.POINTER(TonemapRule), vp, C.c_float, vp, C.POINTER(C.c_float), vp]
            L.pt_tonemap_save_png.argtypes = [vp, C.POINTER(TonemapRule), vp, C.c_float, C.c_char_p, C.POINTER(C.c_float)]
            L.pt_tonemap_srgb_thresholds.argtypes = [vp]
        if hasattr(L, "pt_bloom"):                            # include/pt_bloom.h
            tm, bl = C.POINTER(TonemapRule), C.POINTER(BloomRule)
            L.pt_bloom.argtypes = [vp, bl, ci, vp, C.c_float, vp]
            L.pt_tonemap_bloom.argtypes = [vp, tm, bl, ci, vp, C.c_float, vp, C.POINTER(C.c_float), vp]
            L.pt_tonemap_bloom_save_png.argtypes = [vp, tm, bl, ci, vp, C.c_float, C.c_char_p, C.POINTER(C.c_float)]
        if hasattr(L, "pt_reproject_frame_through"):          # include/pt_reproject_through.h
            L.pt_reproject_frame_through.argtypes = [vp, C.POINTER(ThroughRule), C.POINTER(ReprojectThroughRule), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        if hasattr(L, "pt_reproject_frame_bilinear"):         # include/pt_reproject_bilinear.h
            L.pt_reproject_frame_bilinear.argtypes = [vp, C.POINTER(ReprojectBilinearRule), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        if hasattr(L, "pt_reproject_frame_moved_bilinear"):   # include/pt_motion_bilinear.h
            L.pt_reproject_frame_moved_bilinear.argtypes = [vp, C.POINTER(ReprojectBilinearRule), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        if hasattr(L, "pt_refit_create"):                     # include/pt_refit.h
            L.pt_refit_create.argtypes = [ci, vp, sz, vp, sz, vp, sz, vp, sz, C.c_int64, C.POINTER(vp)]
            L.pt_refit_run.argtypes = [vp, vp, sz, vp, vp]
            L.pt_refit_destroy.argtypes = [vp]
            L.pt_refit_destroy.restype = None
        if hasattr(L, "pt_move_geometry"):                    # include/pt_move.h, and its read-back in include/pt_debug.h
            L.pt_move_geometry.argtypes = [vp, vp, vp, sz, vp, sz, vp, C.POINTER(ci)]
            L.pt_debug_scene_records.argtypes = [vp, ci, vp, sz, C.POINTER(sz)]
        if hasattr(L, "pt_pose_create"):                      # include/pt_pose.h, and its kernel timer in include/pt_debug.h
            L.pt_pose_create.argtypes = [vp, vp, sz, ci, C.POINTER(vp)]
            L.pt_pose_geometry.argtypes = [vp, vp, vp, sz, vp, sz, vp, C.POINTER(ci)]
            L.pt_pose_triangles.argtypes = [vp, vp, sz, vp, sz]
            L.pt_pose_destroy.argtypes = [vp]
            L.pt_pose_destroy.restype = None
            L.pt_debug_pose_time.argtypes = [vp, vp, sz, ci, ci, C.POINTER(C.c_float)]
        if hasattr(L, "pt_skin_create"):                      # include/pt_skin.h, and its kernel timer in include/pt_debug.h
            L.pt_skin_create.argtypes = [vp, vp, sz, vp, sz, ci, C.POINTER(vp)]
            L.pt_debug_skin_time.argtypes = [vp, vp, sz, ci, ci, C.POINTER(C.c_float)]
            L.pt_debug_pose_scratch.argtypes = [vp, vp, sz]
        if hasattr(L, "pt_skin_dq_create"):                   # include/pt_skin_dq.h, and its kernel timer in include/pt_debug.h
            L.pt_skin_dq_create.argtypes = [vp, vp, sz, vp, sz, ci, C.POINTER(vp)]
            L.pt_debug_skin_dq_time.argtypes = [vp, vp, sz, ci, C.POINTER(C.c_float)]
        if hasattr(L, "pt_rig_create"):                       # include/pt_rig.h, and its kernel timer in include/pt_debug.h
            cf, cip = C.c_float, C.POINTER(ci)
            L.pt_rig_create.argtypes = [vp, vp, sz, vp, sz, C.POINTER(vp)]
            L.pt_rig_records.argtypes = [vp, vp, sz, vp, sz]
            L.pt_rig_pose_geometry.argtypes = [vp, vp, vp, sz, vp, sz, vp, cip]
            L.pt_rig_clip_attach.argtypes = [vp, ci, vp, sz, vp, sz]
            L.pt_rig_clip_records.argtypes = [vp, cf, vp, sz]
            L.pt_rig_clip_pose_geometry.argtypes = [vp, vp, cf, vp, sz, vp, cip]
            L.pt_rig_destroy.argtypes = [vp]
            L.pt_rig_destroy.restype = None
            L.pt_debug_rig_time.argtypes = [vp, vp, sz, ci, C.POINTER(cf)]
        if hasattr(L, "pt_rig_mix_clip"):                     # include/pt_rig_mix.h, and its kernel timer in include/pt_debug.h
            cf, cip = C.c_float, C.POINTER(ci)
            L.pt_rig_mix_clip.argtypes = [vp, ci, ci, vp, sz, vp, sz]
            L.pt_rig_mix_mask.argtypes = [vp, ci, vp, sz]
            L.pt_rig_mix_locals.argtypes = [vp, vp, sz, vp, sz]
            L.pt_rig_mix_records.argtypes = [vp, vp, sz, vp, sz]
            L.pt_rig_mix_pose_geometry.argtypes = [vp, vp, vp, sz, vp, sz, vp, cip]
            L.pt_debug_rig_mix_time.argtypes = [vp, vp, sz, ci, C.POINTER(cf)]
        if hasattr(L, "pt_rig_ik_attach"):                    # include/pt_rig_ik.h, and its kernel timer in include/pt_debug.h
            L.pt_rig_ik_attach.argtypes = [vp, vp, sz]
            L.pt_rig_ik_goals.argtypes = [vp, vp, sz]
            L.pt_rig_ik_locals.argtypes = [vp, vp, sz, vp, sz]
            L.pt_debug_rig_ik_time.argtypes = [vp, vp, sz, ci, C.POINTER(C.c_float)]
        if hasattr(L, "pt_morph_attach"):                     # include/pt_morph.h, and its kernel timer and read-back in include/pt_debug.h
            L.pt_morph_attach.argtypes = [vp, ci, vp, sz, vp, sz, vp, sz]
            L.pt_morph_weights.argtypes = [vp, vp, sz]
            L.pt_debug_morph_time.argtypes = [vp, vp, sz, ci, C.POINTER(C.c_float)]
            L.pt_debug_morph_rest.argtypes = [vp, vp, sz]
        if hasattr(L, "pt_normals_attach"):                   # include/pt_normals.h, and its kernel timer in include/pt_debug.h
            L.pt_normals_attach.argtypes = [vp, vp, sz, C.c_int64, C.c_uint32]
            L.pt_normals_mode.argtypes = [vp, ci]
            L.pt_debug_normals_time.argtypes = [vp, vp, sz, ci, ci, C.POINTER(C.c_float)]
        _LIB = L
    return _LIB


class GuidedRule(C.Structure):
    """pt_guided_rule of include/pt_steer.h"""
    _fields_ = [("iterations", C.c_int), ("sigma_lum", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float),
                ("min_frames", C.c_int), ("rel_err", C.c_float), ("abs_err", C.c_float), ("max_frames", C.c_int)]


class ThroughRule(C.Structure):
    """pt_through_rule of include/pt_through.h"""
    _fields_ = [("max_depth", C.c_int), ("min_weight", C.c_float), ("lobes", C.c_int), ("flags", C.c_int)]


class ValidateRule(C.Structure):
    """pt_validate_rule of include/pt_validate.h"""
    _fields_ = [("radius", C.c_int), ("z_lo", C.c_float), ("z_hi", C.c_float), ("normal_tol", C.c_float)]


class DespeckleRule(C.Structure):
    """pt_despeckle_rule of include/pt_despeckle.h"""
    _fields_ = [("radius", C.c_int), ("sigmas", C.c_float), ("min_taps", C.c_int), ("own_z", C.c_float), ("normal_tol", C.c_float), ("min_lum", C.c_float)]


class TonemapRule(C.Structure):
    """pt_tonemap_rule of include/pt_tonemap.h"""
    _fields_ = [("curve", C.c_int), ("transfer", C.c_int), ("exposure", C.c_float), ("key", C.c_float), ("lo_pct", C.c_float), ("hi_pct", C.c_float),
                ("min_exposure", C.c_float), ("max_exposure", C.c_float), ("white", C.c_float), ("adapt", C.c_float)]


TONEMAP_BINS = 512      # PT_TONEMAP_BINS


def tonemap_srgb_thresholds():
    """T of include/pt_tonemap.h's step 5 (pt_tonemap_srgb_thresholds): 256 float32; needs no device"""
    out = np.zeros(256, dtype=np.float32)
    _check(lib().pt_tonemap_srgb_thresholds(out.ctypes.data))
    return out


class BloomRule(C.Structure):
    """pt_bloom_rule of include/pt_bloom.h"""
    _fields_ = [("levels", C.c_int), ("intensity", C.c_float), ("threshold", C.c_float), ("spread", C.c_float)]


BLOOM_SRC_FRAME, BLOOM_SRC_HOST, BLOOM_SRC_FILTERED = 0, 1, 2      # PT_BLOOM_SRC_*
# defaults of bloom_rule: PROVISIONAL — common choices (six levels, a faint glare of the light above an exposed luminance of 1), not tuned on this
# project's workloads
BLOOM_DEFAULTS = dict(levels=6, intensity=0.05, threshold=1.0, spread=0.75)


def bloom_rule(**kw):
    """the pt_bloom_rule of these fields; a field not given takes BLOOM_DEFAULTS'"""
    unknown = set(kw) - set(BLOOM_DEFAULTS)
    assert not unknown, f"no such field of pt_bloom_rule: {sorted(unknown)}"
    v = dict(BLOOM_DEFAULTS, **kw)
    return BloomRule(int(v["levels"]), float(v["intensity"]), float(v["threshold"]), float(v["spread"]))


class ReprojectThroughRule(C.Structure):
    """pt_reproject_through_rule of include/pt_reproject_through.h"""
    _fields_ = [("max_history", C.c_float), ("depth_tol", C.c_float), ("normal_tol", C.c_float), ("point_tol", C.c_float), ("radius", C.c_int),
                ("flags", C.c_int)]


class ReprojectBilinearRule(C.Structure):
    """pt_reproject_bilinear_rule of include/pt_reproject_bilinear.h"""
    _fields_ = [("max_history", C.c_float), ("depth_tol", C.c_float), ("normal_tol", C.c_float), ("snap", C.c_float), ("albedo_floor", C.c_float),
                ("flags", C.c_int)]


class PtError(RuntimeError):
    """Error code + message of the C ABI (the reference throws RuntimeException at these points)."""

    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


def _check(rc):
    if rc != 0:
        raise PtError(rc, lib().pt_last_error().decode())


def shard_slots(W, H, count):
    n = C.c_size_t()
    _check(lib().pt_shard_slots(W, H, count, C.byref(n)))
    return n.value


def shard_map(W, H, rank, count):
    n = shard_slots(W, H, count)
    out = np.empty(n, dtype=np.int32)
    _check(lib().pt_shard_map(W, H, rank, count, out.ctypes.data, n))
    return out


class RefitPlan:
    """A BVH refit plan (include/pt_refit.h): the topology of `buffers` (bindings 10, 11, 12, 13 of a scene; binding 3, when present, gives the
    triangle count) validated, ordered by height and kept on `device`.  run(tris) recomputes binding 10 for a new binding 3 in which triangle k
    is still the same piece of surface (the rule of include/pt_motion.h).  No render context is involved."""

    def __init__(self, buffers, device=0, n_tris=None):
        self._L = lib()
        self._h = C.c_void_p()
        if not hasattr(self._L, "pt_refit_create"):
            raise RuntimeError("this libpt_hip.so has no pt_refit_create (include/pt_refit.h): no fallback")
        data, tree, leaf, roots = (np.ascontiguousarray(buffers[10], dtype=np.float32), np.ascontiguousarray(buffers[11], dtype=np.int32),
                                   np.ascontiguousarray(buffers[12], dtype=np.int32), np.ascontiguousarray(buffers[13], dtype=np.int32))
        self.n_tris = int(n_tris if n_tris is not None else np.asarray(buffers[3]).size // 40)
        self.n_floats, self.n_roots = data.size, int(roots[0]) if roots.size else 0
        _check(self._L.pt_refit_create(int(device), data.ctypes.data, data.nbytes, tree.ctypes.data, tree.nbytes, leaf.ctypes.data, leaf.nbytes,
                                       roots.ctypes.data, roots.nbytes, self.n_tris, C.byref(self._h)))

    def run(self, tris, out=None):
        """-> (binding 10 for these triangles, root_cost: one float64 per root, in binding 13's order).  PtError -4 when a referenced triangle
        holds a NaN; `out`, when given, is then untouched."""
        t = np.ascontiguousarray(tris, dtype=np.float32)
        data = np.empty(self.n_floats, np.float32) if out is None else out
        assert data.dtype == np.float32 and data.size == self.n_floats and data.flags.c_contiguous
        cost = np.zeros(self.n_roots, np.float64)
        _check(self._L.pt_refit_run(self._h, t.ctypes.data, t.nbytes, data.ctypes.data, cost.ctypes.data))
        return data, cost

    def close(self):
        if getattr(self, "_h", None):
            self._L.pt_refit_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pose_records(M, N=None):
    """The 24-float records of include/pt_pose.h for one matrix per part: M is (n_parts, 3, 4) (or 4 x 4, whose last row is dropped), N is
    (n_parts, 3, 3) for the normals.  N not given: the inverse transpose of M's linear part, computed in binary64 and then rounded."""
    M = np.asarray(M, dtype=np.float64)
    if M.ndim == 2:
        M = M[None]
    assert M.ndim == 3 and M.shape[1] in (3, 4) and M.shape[2] == 4, "M must be (n_parts, 3, 4) or (n_parts, 4, 4)"
    M = M[:, :3, :]
    if N is None:
        N = np.transpose(np.linalg.inv(M[:, :, :3]), (0, 2, 1)) if len(M) else np.zeros((0, 3, 3))
    N = np.asarray(N, dtype=np.float64).reshape(-1, 3, 3)
    assert len(N) == len(M), "one N per M"
    out = np.zeros((len(M), 24), np.float32)
    out[:, :12] = M.reshape(len(M), 12)
    out[:, 12:21] = N.reshape(len(M), 9)
    return out


class Pose:
    """A pose object of include/pt_pose.h (Renderer.pose_create): the context's binding 3 as the rest pose, a part id per triangle and a refit plan
    of its own, on the device.  It belongs to its Renderer, whose close() destroys it."""

    def __init__(self, renderer, tri_part, n_parts, skin=None, blend="linear"):
        """skin: (corner_bone, corner_weight) of include/pt_skin.h instead of tri_part (Renderer.skin_create); blend: "linear" for that header's
        rule, "dq" for include/pt_skin_dq.h's"""
        self._L = renderer._L
        self._renderer = renderer                                      # (what a Rig of this pose hands its context from)
        if blend not in ("linear", "dq") or (skin is None and blend != "linear"):
            raise ValueError(f"blend must be 'linear' or 'dq' (and 'dq' needs a skin), not {blend!r}")
        self.blend = blend if skin is not None else None
        name, header = ("pt_pose_create", "include/pt_pose.h") if skin is None else ("pt_skin_create", "include/pt_skin.h")
        if blend == "dq":
            name, header = "pt_skin_dq_create", "include/pt_skin_dq.h"
        if not hasattr(self._L, name):
            raise RuntimeError(f"this libpt_hip.so has no {name} ({header}): no fallback")
        self._h = C.c_void_p()
        if skin is None:
            part = np.ascontiguousarray(tri_part, dtype=np.int32)
            self.n_parts, self.n_tris, self.n_roots = int(n_parts), part.size, getattr(renderer, "_n_roots", 0)
            _check(self._L.pt_pose_create(renderer._h, part.ctypes.data, part.nbytes, self.n_parts, C.byref(self._h)))
            return
        bone = np.ascontiguousarray(skin[0], dtype=np.int32).reshape(-1)
        weight = np.ascontiguousarray(skin[1], dtype=np.float32).reshape(-1)
        self.n_parts, self.n_tris, self.n_roots = int(n_parts), bone.size // 12, getattr(renderer, "_n_roots", 0)
        create = self._L.pt_skin_dq_create if blend == "dq" else self._L.pt_skin_create
        _check(create(renderer._h, bone.ctypes.data, bone.nbytes, weight.ctypes.data, weight.nbytes, self.n_parts, C.byref(self._h)))

    def _xforms(self, xforms):
        x = np.ascontiguousarray(xforms, dtype=np.float32).reshape(-1)
        return x, (x.ctypes.data if x.size else None)

    def triangles(self, xforms):
        """the posed binding 3 (the rule alone: nothing of the context changes)"""
        x, xp = self._xforms(xforms)
        out = np.empty(self.n_tris * 40, np.float32)
        _check(self._L.pt_pose_triangles(self._h, xp, x.nbytes, out.ctypes.data, out.nbytes))
        return out

    def morph_attach(self, targets):
        """Attach morph targets (pt_morph_attach, include/pt_morph.h): targets is a list of (corners int32[m], deltas float32[m, 6]) — corner
        3 * k + c of triangle k, and dx dy dz for its vertex, dnx dny dnz for its normal.  Once per pose; every weight is 0 afterwards."""
        if not hasattr(self._L, "pt_morph_attach"):
            raise RuntimeError("this libpt_hip.so has no pt_morph_attach (include/pt_morph.h): no fallback")
        corners = [np.ascontiguousarray(c, dtype=np.int32).reshape(-1) for c, _ in targets]
        deltas = [np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 6) for _, d in targets]
        assert all(len(c) == len(d) for c, d in zip(corners, deltas)), "one delta of 6 floats per corner"
        start = np.zeros(len(targets) + 1, np.int64)
        start[1:] = np.cumsum([c.size for c in corners])
        corner = np.concatenate(corners + [np.zeros(0, np.int32)])
        delta = np.concatenate(deltas + [np.zeros((0, 6), np.float32)]).reshape(-1)
        _check(self._L.pt_morph_attach(self._h, len(targets), start.ctypes.data, start.nbytes, corner.ctypes.data, corner.nbytes, delta.ctypes.data, delta.nbytes))
        self.n_targets = len(targets)

    def morph_weights(self, w):
        """one weight per target for the next Renderer.pose_geometry and Pose.triangles (pt_morph_weights)"""
        if not hasattr(self._L, "pt_morph_weights"):
            raise RuntimeError("this libpt_hip.so has no pt_morph_weights (include/pt_morph.h): no fallback")
        w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
        _check(self._L.pt_morph_weights(self._h, w.ctypes.data, w.nbytes))

    def normals_attach(self, corner_vertex, n_vertices=None, flip=False):
        """Attach recomputed normals (pt_normals_attach, include/pt_normals.h): corner_vertex holds one id per corner (3 per triangle), -1 for a
        corner that keeps the pose rule's normal; corners with the same id >= 0 are one vertex and get the same normal.  n_vertices: one more
        than the largest id when not given.  Once per pose; the mode is 1 afterwards."""
        if not hasattr(self._L, "pt_normals_attach"):
            raise RuntimeError("this libpt_hip.so has no pt_normals_attach (include/pt_normals.h): no fallback")
        ids = np.ascontiguousarray(corner_vertex, dtype=np.int32).reshape(-1)
        if n_vertices is None:
            n_vertices = int(ids.max()) + 1 if ids.size else 0
        _check(self._L.pt_normals_attach(self._h, ids.ctypes.data, ids.nbytes, int(n_vertices), 1 if flip else 0))
        self.n_vertices = int(n_vertices)

    def normals_mode(self, on):
        """0: the pose rule's normals, 1: recomputed, for the next Renderer.pose_geometry and Pose.triangles (pt_normals_mode)"""
        if not hasattr(self._L, "pt_normals_mode"):
            raise RuntimeError("this libpt_hip.so has no pt_normals_mode (include/pt_normals.h): no fallback")
        _check(self._L.pt_normals_mode(self._h, int(on)))

    def rig(self, parent, inv_bind=None):
        """A Rig over this pose (pt_rig_create, include/pt_rig.h): parent[j] in [-1, j) per record of the pose, inv_bind (n_parts, 3, 4) or None.
        It makes this pose's records on the device from local joint transforms or from a time into a keyed clip."""
        return Rig(self, parent, inv_bind)

    def close(self):
        if getattr(self, "_h", None):
            self._L.pt_pose_destroy(self._h)
            self._h = None


def rig_locals(t=None, q=None, s=None, n=None):
    """The 12-float locals of include/pt_rig.h for n joints: t (n, 3) translations (default 0), q (n, 4) quaternions as x y z w (default the
    identity), s (n, 3) scales (default 1); the two padding floats are 0."""
    given = [np.asarray(a) for a in (t, q, s) if a is not None]
    n = int(n if n is not None else (given[0].reshape(-1, given[0].shape[-1]).shape[0] if given else 0))
    out = np.zeros((n, 12), np.float32)
    out[:, 7] = 1.0
    out[:, 8:11] = 1.0
    if t is not None:
        out[:, 0:3] = np.asarray(t, np.float64).reshape(n, 3)
    if q is not None:
        out[:, 4:8] = np.asarray(q, np.float64).reshape(n, 4)
    if s is not None:
        out[:, 8:11] = np.asarray(s, np.float64).reshape(n, 3)
    return out


RIG_LAYER = np.dtype([("clip", np.int32), ("mask", np.int32), ("mode", np.int32), ("wrap", np.int32), ("t", np.float32), ("weight", np.float32)])      # pt_rig_layer, 24 bytes
RIG_MIX_MODES = {"override": 0, "additive": 1}
RIG_MIX_WRAPS = {"clamp": 0, "loop": 1}


def rig_layers(layers):
    """The 24-byte layer records of include/pt_rig_mix.h from a list of tuples (clip, t[, weight[, mask[, mode[, wrap]]]]) or dicts with those
    keys; weight defaults to 1, mask to -1 (none), mode to "override" (or "additive", or the number), wrap to "clamp" (or "loop", or the
    number).  An array of RIG_LAYER passes through."""
    if isinstance(layers, np.ndarray) and layers.dtype == RIG_LAYER:
        return np.ascontiguousarray(layers).reshape(-1)
    names = ("clip", "t", "weight", "mask", "mode", "wrap")
    out = np.zeros(len(layers), RIG_LAYER)
    for i, y in enumerate(layers):
        d = dict(weight=1.0, mask=-1, mode=0, wrap=0)
        d.update(y if isinstance(y, dict) else dict(zip(names, y)))
        unknown = set(d) - set(names)
        if unknown or "clip" not in d or "t" not in d:
            raise ValueError(f"rig_layers: layer {i} needs clip and t and knows {names}")
        mode, wrap = d["mode"], d["wrap"]
        out[i] = (int(d["clip"]), int(d["mask"]), RIG_MIX_MODES[mode] if isinstance(mode, str) else int(mode), RIG_MIX_WRAPS[wrap] if isinstance(wrap, str) else int(wrap),
                  np.float32(d["t"]), np.float32(d["weight"]))
    return out


RIG_IK_CONSTRAINT = np.dtype([("kind", np.int32), ("joint", np.int32), ("flags", np.int32), ("pad", np.int32), ("axis", np.float32, 3), ("padf", np.float32)])      # 32 bytes
RIG_IK_GOAL = np.dtype([("target", np.float32, 3), ("weight", np.float32), ("pole", np.float32, 3), ("padf", np.float32)])      # pt_rig_ik_goal, 32 bytes
RIG_IK_KINDS = {"two_bone": 0, "aim": 1}
RIG_IK_POLE = 1


def rig_ik_constraints(constraints):
    """The 32-byte constraint records of include/pt_rig_ik.h from a list of tuples (kind, joint[, pole[, axis]]) or dicts with those keys: kind
    "two_bone" (joint is the tip) or "aim" (or the number), pole whether a two-bone goal's pole is read, axis the aim's unit axis in the
    joint's frame.  An array of RIG_IK_CONSTRAINT passes through."""
    if isinstance(constraints, np.ndarray) and constraints.dtype == RIG_IK_CONSTRAINT:
        return np.ascontiguousarray(constraints).reshape(-1)
    names = ("kind", "joint", "pole", "axis")
    out = np.zeros(len(constraints), RIG_IK_CONSTRAINT)
    for i, c in enumerate(constraints):
        d = dict(pole=False, axis=(0.0, 0.0, 0.0))
        d.update(c if isinstance(c, dict) else dict(zip(names, c)))
        if set(d) - set(names) or "kind" not in d or "joint" not in d:
            raise ValueError(f"rig_ik_constraints: constraint {i} needs kind and joint and knows {names}")
        kind = d["kind"]
        out[i] = (RIG_IK_KINDS[kind] if isinstance(kind, str) else int(kind), int(d["joint"]), RIG_IK_POLE if d["pole"] else 0, 0, np.asarray(d["axis"], np.float32), 0.0)
    return out


def rig_ik_goals(goals):
    """The 32-byte goal records of include/pt_rig_ik.h, one per constraint, from a list of tuples (target[, weight[, pole]]) or dicts with those
    keys, in world space; weight defaults to 1.  An array of RIG_IK_GOAL passes through."""
    if isinstance(goals, np.ndarray) and goals.dtype == RIG_IK_GOAL:
        return np.ascontiguousarray(goals).reshape(-1)
    names = ("target", "weight", "pole")
    out = np.zeros(len(goals), RIG_IK_GOAL)
    for i, g in enumerate(goals):
        d = dict(weight=1.0, pole=(0.0, 0.0, 0.0))
        d.update(g if isinstance(g, dict) else dict(zip(names, g)))
        if set(d) - set(names) or "target" not in d:
            raise ValueError(f"rig_ik_goals: goal {i} needs target and knows {names}")
        out[i] = (np.asarray(d["target"], np.float32), np.float32(d["weight"]), np.asarray(d["pole"], np.float32), 0.0)
    return out


class Rig:
    """A rig of include/pt_rig.h (Pose.rig): a joint per record of its pose, evaluated on the device.  It belongs to its Pose, whose close()
    destroys it, as the Renderer's does."""

    def __init__(self, pose, parent, inv_bind=None):
        self._L, self._pose = pose._L, pose
        if not hasattr(self._L, "pt_rig_create"):
            raise RuntimeError("this libpt_hip.so has no pt_rig_create (include/pt_rig.h): no fallback")
        p = np.ascontiguousarray(parent, dtype=np.int32).reshape(-1)
        b = None if inv_bind is None else np.ascontiguousarray(inv_bind, dtype=np.float32).reshape(-1)
        self.n_parts, self.n_roots = pose.n_parts, pose.n_roots
        self._h = C.c_void_p()
        _check(self._L.pt_rig_create(pose._h, p.ctypes.data, p.nbytes, None if b is None else b.ctypes.data, 0 if b is None else b.nbytes, C.byref(self._h)))

    @staticmethod
    def _floats(a):
        x = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        return x, (x.ctypes.data if x.size else None)

    def records(self, locals):
        """the records of these locals (n_parts x 12 floats: rig_locals), (n_parts, 24): the rule alone (pt_rig_records)"""
        l, lp = self._floats(locals)
        out = np.empty((self.n_parts, 24), np.float32)
        _check(self._L.pt_rig_records(self._h, lp, l.nbytes, out.ctypes.data, out.nbytes))
        return out

    def _geometry(self, call, *args, ellip=None):
        e = None if ellip is None else np.ascontiguousarray(ellip, dtype=np.float32)
        cost = np.zeros(self.n_roots, np.float64)
        in_place = C.c_int(-1)
        _check(call(self._pose._renderer._h, self._h, *args, None if e is None else e.ctypes.data, 0 if e is None else e.nbytes, cost.ctypes.data, C.byref(in_place)))
        return cost, bool(in_place.value)

    def pose(self, locals, ellip=None):
        """Renderer.pose_geometry of the pose under the records of these locals, made on the device (pt_rig_pose_geometry): no record is
        uploaded.  Returns (root_cost, in_place)."""
        l, lp = self._floats(locals)
        return self._geometry(self._L.pt_rig_pose_geometry, lp, l.nbytes, ellip=ellip)

    def clip(self, times, values):
        """Attach a keyed clip (pt_rig_clip_attach): times (n_keys,) strictly increasing, values (n_keys, n_parts, 12) locals.  A second clip
        replaces the first."""
        t, tp = self._floats(times)
        v, vp = self._floats(values)
        _check(self._L.pt_rig_clip_attach(self._h, t.size, tp, t.nbytes, vp, v.nbytes))
        self.n_keys = t.size

    def records_at(self, t):
        """the records of the clip at time t (pt_rig_clip_records): a normalised lerp between the two keys around t, clamped to the clip"""
        out = np.empty((self.n_parts, 24), np.float32)
        _check(self._L.pt_rig_clip_records(self._h, float(t), out.ctypes.data, out.nbytes))
        return out

    def pose_at(self, t, ellip=None):
        """Rig.pose with the clip's records at time t (pt_rig_clip_pose_geometry): the step uploads one float"""
        return self._geometry(self._L.pt_rig_clip_pose_geometry, float(t), ellip=ellip)

    def _mix_call(self, name):
        if not hasattr(self._L, name):
            raise RuntimeError(f"this libpt_hip.so has no {name} (include/pt_rig_mix.h): no fallback")
        return getattr(self._L, name)

    def mix_clip(self, slot, times, values):
        """Fill clip slot `slot` of include/pt_rig_mix.h (pt_rig_mix_clip): times and values as Rig.clip takes them.  A second attach to a
        slot replaces the first; Rig.clip's own clip is another thing."""
        t, tp = self._floats(times)
        v, vp = self._floats(values)
        _check(self._mix_call("pt_rig_mix_clip")(self._h, int(slot), t.size, tp, t.nbytes, vp, v.nbytes))

    def mask(self, slot, weights):
        """Fill mask slot `slot` (pt_rig_mix_mask): one weight in [0, 1] per joint"""
        w, wp = self._floats(weights)
        _check(self._mix_call("pt_rig_mix_mask")(self._h, int(slot), wp, w.nbytes))

    def mix_locals(self, layers):
        """the mixed locals of these layers (rig_layers, or what it takes), (n_parts, 12): the mix alone (pt_rig_mix_locals)"""
        y = rig_layers(layers)
        out = np.empty((self.n_parts, 12), np.float32)
        _check(self._mix_call("pt_rig_mix_locals")(self._h, y.ctypes.data if y.size else None, y.nbytes, out.ctypes.data, out.nbytes))
        return out

    def mix_records(self, layers):
        """the records of the mixed locals, (n_parts, 24) (pt_rig_mix_records)"""
        y = rig_layers(layers)
        out = np.empty((self.n_parts, 24), np.float32)
        _check(self._mix_call("pt_rig_mix_records")(self._h, y.ctypes.data if y.size else None, y.nbytes, out.ctypes.data, out.nbytes))
        return out

    def mix(self, layers, ellip=None):
        """Rig.pose with the records of the mixed locals (pt_rig_mix_pose_geometry): the step uploads the layers, 24 bytes each"""
        y = rig_layers(layers)
        return self._geometry(self._mix_call("pt_rig_mix_pose_geometry"), y.ctypes.data if y.size else None, y.nbytes, ellip=ellip)

    def _ik_call(self, name):
        if not hasattr(self._L, name):
            raise RuntimeError(f"this libpt_hip.so has no {name} (include/pt_rig_ik.h): no fallback")
        return getattr(self._L, name)

    def ik(self, constraints):
        """Attach the constraint table of include/pt_rig_ik.h (pt_rig_ik_attach): rig_ik_constraints, or what it takes.  It replaces the table
        (an empty list: none) and clears the goals."""
        c = rig_ik_constraints(constraints)
        _check(self._ik_call("pt_rig_ik_attach")(self._h, c.ctypes.data if c.size else None, c.nbytes))
        self.n_constraints = c.size

    def ik_goals(self, goals):
        """Set the goals (pt_rig_ik_goals), one per constraint, in world space: rig_ik_goals, or what it takes.  While they are set every
        record call of the rig solves the constraints between its source and its levels.  None: off."""
        if goals is None:
            _check(self._ik_call("pt_rig_ik_goals")(self._h, None, 0))
            return
        g = rig_ik_goals(goals)
        keep = np.zeros(1, RIG_IK_GOAL)                          # (an empty array of goals is not None: goals for an empty table)
        _check(self._ik_call("pt_rig_ik_goals")(self._h, g.ctypes.data if g.size else keep.ctypes.data, g.nbytes))

    def ik_locals(self, locals):
        """these locals after the solve under the goals set, (n_parts, 12): the rule alone (pt_rig_ik_locals)"""
        l, lp = self._floats(locals)
        out = np.empty((self.n_parts, 12), np.float32)
        _check(self._ik_call("pt_rig_ik_locals")(self._h, lp, l.nbytes, out.ctypes.data, out.nbytes))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.pt_rig_destroy(self._h)
            self._h = None


class Renderer:
    """One render context.  `devices=[...]`: ONE context made of several wavefront streams (pt_create_multi): one entry per stream —
    several GPUs ([0, 1, ...]), several independent streams on one GPU ([0, 0]: their kernels overlap, 11-24 % faster than one: include/pt_api.h), or both
    ([0, 0, 1, 1]); the tile shards, the per-stream host threads and the gather of every image live inside the library.
    first_shard / total_shards: the group renders only shards first_shard.. of total_shards (one process per GPU; pt_create_multi_part)."""

    def __init__(self, W, H, device=0, shard_rank=0, shard_count=1, devices=None, first_shard=0, total_shards=None):
        self._L = lib()
        self._h = C.c_void_p()
        self.W, self.H, self.shard_rank, self.shard_count = W, H, shard_rank, shard_count
        self.devices = None if devices is None else [int(d) for d in devices]
        if self.devices is not None:
            assert shard_count == 1 and shard_rank == 0, "a multi-stream context shards by itself"
            arr = (C.c_int * len(self.devices))(*self.devices)
            self.first_shard, self.total_shards = int(first_shard), int(total_shards if total_shards is not None else len(self.devices))
            _check(self._L.pt_create_multi_part(C.byref(self._h), arr, len(self.devices), W, H, self.first_shard, self.total_shards))
            note = self._L.pt_last_error().decode()
            if note.startswith("warning:"):
                import warnings
                warnings.warn(note[len("warning:"):].strip())
        else:
            _check(self._L.pt_create(C.byref(self._h), device, W, H, shard_rank, shard_count))

    def close(self):
        if getattr(self, "_h", None):
            self._L.pt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- SSBO / texture uploads -------------------------------------------------------------
    def set_buffer(self, binding, array):
        a = np.ascontiguousarray(array)
        assert a.dtype in (np.float32, np.int32), "SSBO contents are float32 or int32"
        _check(self._L.pt_set_buffer(self._h, int(binding), a.ctypes.data, a.nbytes))
        if int(binding) == 13:
            self._n_roots = int(a.reshape(-1)[0]) if a.size else 0      # (what a Pose's root_cost is sized by)

    def set_texture(self, index, rgba8):
        a = np.ascontiguousarray(rgba8, dtype=np.uint8)
        assert a.ndim == 3 and a.shape[2] == 4
        _check(self._L.pt_set_texture(self._h, int(index), a.shape[1], a.shape[0], a.ctypes.data))

    def load_workload(self, wl):
        for b, arr in wl.buffers.items():
            self.set_buffer(b, arr)
        self.set_texture(0, wl.sky)
        for idx, arr in getattr(wl, "textures", {}).items():
            self.set_texture(idx, arr)

    # --- frame loop ---------------------------------------------------------------------------
    def reset_frame(self):
        _check(self._L.pt_reset_frame(self._h))

    def render(self, frame_count, seed):
        _check(self._L.pt_render(self._h, int(frame_count), int(seed)))

    def render_batch(self, first_frame, seeds):
        s = np.ascontiguousarray(seeds, dtype=np.int32)
        _check(self._L.pt_render_batch(self._h, int(first_frame), int(s.size), s.ctypes.data))

    # overlapped batches: the path pool keeps running from one batch into the next (include/pt_api.h)
    def render_batch_async(self, first_frame, seeds):
        s = np.ascontiguousarray(seeds, dtype=np.int32)
        _check(self._L.pt_render_batch_async(self._h, int(first_frame), int(s.size), s.ctypes.data))

    def next_image(self):
        _check(self._L.pt_next_image(self._h))

    def finish_image(self, age=0):
        _check(self._L.pt_finish_image(self._h, int(age)))

    def image_device(self, age=0):
        p, n = C.c_void_p(), C.c_size_t()
        _check(self._L.pt_image_device(self._h, int(age), C.byref(p), C.byref(n)))
        return p.value, n.value

    def gather_image(self, age=0):
        """Device pointer of the whole W x H RGBA32F image `age` images ago: on a multi-GPU context this is the ONE RCCL gather
        + un-tiling on devices[0] (stream-ordered there, not synchronised)."""
        p = C.c_void_p()
        _check(self._L.pt_gather_image(self._h, int(age), C.byref(p)))
        return p.value

    def synchronize(self):
        _check(self._L.pt_synchronize(self._h))

    def stream_wait(self):
        """wait for what is enqueued on the context's stream(s) (gather, un-tiling, accumulation) without completing batches in flight"""
        _check(self._L.pt_stream_wait(self._h))

    def read_frame(self, out=None):
        if out is None:
            out = np.zeros((self.H, self.W, 4), dtype=np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == self.W * self.H * 4
        _check(self._L.pt_read_frame(self._h, out.ctypes.data))
        return out

    def write_frame(self, frame):
        """restore a saved FRAME image (running sum + count): the next frames accumulate on top of it (pt_write_frame)"""
        frame = np.ascontiguousarray(frame, dtype=np.float32)
        assert frame.size == self.W * self.H * 4
        _check(self._L.pt_write_frame(self._h, frame.ctypes.data))

    def read_display(self, frame_count, java_bytes=True):
        """The reference's screenshot image: (H, W, 3) uint8, top row first (functions.screenshot, dispatch.java:804-851)."""
        out = np.zeros((self.H, self.W, 3), dtype=np.uint8)
        _check(self._L.pt_read_display(self._h, int(frame_count), 1 if java_bytes else 0, out.ctypes.data))
        return out

    # --- adaptive sampling (include/pt_adaptive.h) -----------------------------------------------
    def render_adaptive(self, first_frame, seeds, rel_err, abs_err=0.0, min_frames=4, max_frames=0):
        """Frames first_frame.. (one per seed) for the pixels whose per-pixel luminance statistics still say noisy (pt_render_adaptive);
        returns how many pixels were rendered.  FRAME alpha then holds every pixel's own frame count: show it with read_display_mean."""
        s = np.ascontiguousarray(seeds, dtype=np.int32)
        n = C.c_int64(0)
        _check(self._L.pt_render_adaptive(self._h, int(first_frame), int(s.size), s.ctypes.data, float(rel_err), float(abs_err),
                                          int(min_frames), int(max_frames), C.byref(n)))
        return n.value

    def read_display_mean(self, java_bytes=True):
        """read_display with every pixel divided by its own frame count (FRAME alpha): (H, W, 3) uint8, top row first"""
        out = np.zeros((self.H, self.W, 3), dtype=np.uint8)
        _check(self._L.pt_read_display_mean(self._h, 1 if java_bytes else 0, out.ctypes.data))
        return out

    # --- first-hit features and the denoised image (include/pt_denoise.h) -------------------------
    # default sigmas of denoise / read_display_denoised (colour, normal, depth, albedo): the lowest RMSE of scripts/denoise_quality.py's grid on C3
    # and C6 at 1080p, 4 and 16 frames (profiles/r09_denoise_quality.txt)
    DENOISE_SIGMAS = (4.0, 0.3, 0.05, 0.1)

    def read_features(self):
        """the raw feature records (pt_read_features): (H, W, 16) float32, FRAME order (row 0 = y 0)"""
        out = np.zeros((self.H, self.W, 16), dtype=np.float32)
        _check(self._L.pt_read_features(self._h, out.ctypes.data))
        return out

    def features(self):
        """first-hit feature buffers of the lens-centre camera ray of every pixel, as (H, W[, k]) arrays: t (rayScene's distance, -1 on a miss),
        normal (before the face-forward flip), albedo (Kd after mapMtl), hit (type * 0x1000000 + id, -1 on a miss), dir, material (-1 on a miss), uv"""
        f = self.read_features()
        return {"t": f[..., 0].copy(), "normal": f[..., 1:4].copy(), "albedo": f[..., 4:7].copy(), "hit": f[..., 7].copy().view(np.int32),
                "dir": f[..., 8:11].copy(), "material": f[..., 11].copy().view(np.int32), "uv": f[..., 12:14].copy()}

    def _sigmas(self, sigma_color, sigma_normal, sigma_depth, sigma_albedo):
        d = self.DENOISE_SIGMAS
        return [float(d[k] if v is None else v) for k, v in enumerate((sigma_color, sigma_normal, sigma_depth, sigma_albedo))]

    def denoise(self, iterations=5, sigma_color=None, sigma_normal=None, sigma_depth=None, sigma_albedo=None):
        """the edge-avoiding a-trous filter over FRAME.rgb / FRAME.a (pt_denoise): (H, W, 4) float32, rgb = denoised mean, a = FRAME.a.
        FRAME is not modified.  A sigma of None takes DENOISE_SIGMAS; float('inf') switches its term off."""
        out = np.zeros((self.H, self.W, 4), dtype=np.float32)
        _check(self._L.pt_denoise(self._h, int(iterations), *self._sigmas(sigma_color, sigma_normal, sigma_depth, sigma_albedo), out.ctypes.data))
        return out

    def read_display_denoised(self, iterations=5, sigma_color=None, sigma_normal=None, sigma_depth=None, sigma_albedo=None, java_bytes=True):
        """denoise()'s image converted to 8 bits as read_display converts a mean: (H, W, 3) uint8, top row first"""
        out = np.zeros((self.H, self.W, 3), dtype=np.uint8)
        _check(self._L.pt_read_display_denoised(self._h, int(iterations), *self._sigmas(sigma_color, sigma_normal, sigma_depth, sigma_albedo),
                                                1 if java_bytes else 0, out.ctypes.data))
        return out

    # --- reprojection across a camera move (include/pt_reproject.h) --------------------------------
    REPROJECT_ALL_MATERIALS = 1

    def reproject_frame(self, max_history=64, depth_tol=0.02, normal_tol=0.9, all_materials=False, albedo_floor=None):
        """Carry the current image across the camera move since it was rendered (pt_reproject_frame): every pixel of the current view takes over
        the sum and count of the old pixel that saw the same surface point, capped at max_history frames; the others restart from zero.
        Returns how many pixels kept their history.  Continue with frame numbers other than 1 and show the image with read_display_mean.
        The defaults: scripts/reproject_quality.py on C2 and C3 at 1080p (profiles/r10_reproject_quality.txt).
        albedo_floor: a number carries illumination and gives every pixel its own albedo back (pt_reproject_frame_demod, include/pt_demod.h)."""
        n = C.c_int64(0)
        flags = self.REPROJECT_ALL_MATERIALS if all_materials else 0
        if albedo_floor is None:
            _check(self._L.pt_reproject_frame(self._h, float(max_history), float(depth_tol), float(normal_tol), flags, C.byref(n)))
        else:
            _check(self._L.pt_reproject_frame_demod(self._h, float(max_history), float(depth_tol), float(normal_tol), flags, float(albedo_floor), C.byref(n)))
        return n.value

    # --- reprojection of mirror and glass pixels through their chains (include/pt_reproject_through.h) ---
    # defaults of reproject_through_rule: the float32 model on the oracle's frames of C3 at 160 x 90 (tests/test_reproject_through_abi.py, DESIGN.md
    # 2.17): 32 frames, move(forward 0.05, strafe 0.03, yaw 0.02), 4 frames, clamped RMSE over the 1941 chain pixels against 128 frames.  Of the
    # grid point_tol (0.01, 0.02, 0.05) x radius (0, 1, 2, 4), (0.05, 2) is best: 0.0798 against 0.1580 for pt_reproject_frame, which restarts
    # there; (0.02, 2) gives 0.1039, (0.05, 0) 0.1142, (0.05, 4) 0.0823.
    REPROJECT_THROUGH_POINT_TOL = 0.05
    REPROJECT_THROUGH_RADIUS = 2
    REPROJECT_THROUGH_CHAINS = (4, 0.5, 3, True)                  # the through_rule it follows: depth 4, both lobes at 0.5, with the key (required)

    def reproject_through_rule(self, max_history=64.0, depth_tol=0.02, normal_tol=0.9, point_tol=None, radius=None, all_materials=False):
        """the pt_reproject_through_rule of these arguments; None takes the defaults above, the first three are reproject_frame's"""
        return ReprojectThroughRule(float(max_history), float(depth_tol), float(normal_tol),
                                    float(self.REPROJECT_THROUGH_POINT_TOL if point_tol is None else point_tol),
                                    int(self.REPROJECT_THROUGH_RADIUS if radius is None else radius), self.REPROJECT_ALL_MATERIALS if all_materials else 0)

    def reproject_frame_through(self, thru=None, rule=None):
        """reproject_frame that also carries the pixels of mirrors and glass (pt_reproject_frame_through): a pixel with a seen-through chain under
        `thru` (a through_rule() with the key) takes the history of the old pixel whose chain ended on the same surface point, searched in a
        window around the projected virtual point.  Returns (kept, kept_through): the pixels that kept their history, and those among them
        with a chain.  None takes REPROJECT_THROUGH_CHAINS and reproject_through_rule()."""
        thru = self.through_rule(*self.REPROJECT_THROUGH_CHAINS) if thru is None else thru
        rule = self.reproject_through_rule() if rule is None else rule
        n, nt = C.c_int64(0), C.c_int64(0)
        _check(self._L.pt_reproject_frame_through(self._h, C.byref(thru), C.byref(rule), C.byref(n), C.byref(nt)))
        return n.value, nt.value

    # --- reprojection with bilinear taps (include/pt_reproject_bilinear.h) --------------------------
    def reproject_frame_bilinear(self, max_history=64, depth_tol=0.02, normal_tol=0.9, snap=1 / 64, all_materials=False, albedo_floor=0.0):
        """reproject_frame that blends the qualifying old pixels around the projected point with bilinear weights (pt_reproject_frame_bilinear)
        where reproject_frame copies the nearest one: no half-pixel snapping under a slow move, and a pixel restarts only when none of its up
        to four taps passes.  snap: a projected point closer than this (in pixels) to an old pixel's centre is that pixel, which keeps an
        unchanged camera the identity; the default stays far above the rounding of the projection.  albedo_floor 0: the plain
        carry; > 0: include/pt_demod.h's.  Returns (kept, blended): the pixels that kept history, and those among them blended from two or
        more old pixels.  Counts become fractional, as after history_merge."""
        rule = ReprojectBilinearRule(float(max_history), float(depth_tol), float(normal_tol), float(snap), float(albedo_floor),
                                     self.REPROJECT_ALL_MATERIALS if all_materials else 0)
        n, nb = C.c_int64(0), C.c_int64(0)
        _check(self._L.pt_reproject_frame_bilinear(self._h, C.byref(rule), C.byref(n), C.byref(nb)))
        return n.value, nb.value

    # --- reprojection across moved geometry (include/pt_motion.h) ----------------------------------
    def motion_mark(self):
        """Pin the scene the current image was rendered in (pt_motion_mark): call it before uploading moved geometry (bindings 3, 7, 10-13)."""
        _check(self._L.pt_motion_mark(self._h))

    def reproject_frame_moved(self, max_history=64.0, depth_tol=0.02, normal_tol=0.9, all_materials=False, albedo_floor=0.0):
        """reproject_frame across the geometry uploaded since motion_mark (pt_reproject_frame_moved): every pixel follows its surface point back
        to where its primitive was at the mark.  Triangle k and ellipsoid k must be the same piece of surface as at the mark.  albedo_floor 0:
        the plain carry; > 0: include/pt_demod.h's.  Returns the kept count; the mark is spent.  Defaults: reproject_frame's
        (scripts/motion_quality.py)."""
        n = C.c_int64(0)
        flags = self.REPROJECT_ALL_MATERIALS if all_materials else 0
        _check(self._L.pt_reproject_frame_moved(self._h, float(max_history), float(depth_tol), float(normal_tol), flags, float(albedo_floor), C.byref(n)))
        return n.value

    # --- BVH refit for moved triangles (include/pt_refit.h) -----------------------------------------
    def move_triangles(self, plan, tris):
        """Upload a moved binding 3 and the binding 10 that `plan` (a RefitPlan over this scene's bindings 10-13) refits to it; bindings 11-13 stay
        as uploaded.  Between motion_mark and reproject_frame_moved this replaces the rebuild of every tree; moved ellipsoids (binding 7) are the
        caller's to upload.  Returns (binding 10, root_cost): the cost against the rest pose's says when a rebuild pays."""
        data, cost = plan.run(tris)
        self.set_buffer(3, np.ascontiguousarray(tris, dtype=np.float32))
        self.set_buffer(10, data)
        return data, cost

    # --- triangles moved in place (include/pt_move.h) ------------------------------------------------
    def move_geometry(self, plan, tris, ellip=None):
        """move_triangles (and set_buffer(7, ellip) when `ellip` is given) with the context's device records patched in place
        (pt_move_geometry): the refit runs, and what of the built scene depends on the triangles' coordinates and the trees' boxes is rewritten on
        the device from the plan's copies, so the next render neither lays the scene out again nor uploads its record arrays.  The context ends
        in the state move_triangles and the next render's scene build would leave it in.  Returns (root_cost, in_place): in_place is False when
        the call had to build the scene after all (a multi-stream context, foreign unordered boxes, a binding 7 that changes a count or a
        material)."""
        if not hasattr(self._L, "pt_move_geometry"):
            raise RuntimeError("this libpt_hip.so has no pt_move_geometry (include/pt_move.h): no fallback")
        t = np.ascontiguousarray(tris, dtype=np.float32)
        e = None if ellip is None else np.ascontiguousarray(ellip, dtype=np.float32)
        cost = np.zeros(plan.n_roots, np.float64)
        in_place = C.c_int(-1)
        _check(self._L.pt_move_geometry(self._h, plan._h, t.ctypes.data, t.nbytes, None if e is None else e.ctypes.data, 0 if e is None else e.nbytes,
                                        cost.ctypes.data, C.byref(in_place)))
        return cost, bool(in_place.value)

    # --- triangles animated by per-part matrices on the device (include/pt_pose.h) -------------------
    pose_records = staticmethod(pose_records)

    def pose_create(self, tri_part, n_parts):
        """A Pose over this context's scene as it is now (pt_pose_create): binding 3 is the rest pose, tri_part[k] in [-1, n_parts) the part of
        triangle k (-1: static)."""
        return Pose(self, tri_part, n_parts)

    def skin_create(self, corner_bone, corner_weight, n_parts, blend="linear"):
        """A skinned Pose over this context's scene as it is now (pt_skin_create, include/pt_skin.h): 12 bone ids and 12 weights per triangle,
        corner c, slot s at 12*k + 4*c + s; a corner's used slots first, -1 in the others; a corner without slots is static.  pose_geometry,
        Pose.triangles and pose_records work on it as on a Pose of pose_create.  blend="dq": the same tables under the dual-quaternion rule
        (pt_skin_dq_create, include/pt_skin_dq.h), which keeps the volume of what twists; Pose.blend carries the choice."""
        return Pose(self, None, n_parts, skin=(corner_bone, corner_weight), blend=blend)

    def pose_geometry(self, pose, xforms, ellip=None):
        """move_geometry of the rest pose under `xforms` (n_parts records of 24 floats: pose_records), with the posed triangles, the refit and the
        patch of the records made on the device (pt_pose_geometry): no triangle data crosses the bus; the host copies of bindings 3 and 10 are
        brought up to date when something reads them.  Returns (root_cost, in_place) as move_geometry does."""
        if not hasattr(self._L, "pt_pose_geometry"):
            raise RuntimeError("this libpt_hip.so has no pt_pose_geometry (include/pt_pose.h): no fallback")
        x, xp = pose._xforms(xforms)
        e = None if ellip is None else np.ascontiguousarray(ellip, dtype=np.float32)
        cost = np.zeros(pose.n_roots, np.float64)
        in_place = C.c_int(-1)
        _check(self._L.pt_pose_geometry(self._h, pose._h, xp, x.nbytes, None if e is None else e.ctypes.data, 0 if e is None else e.nbytes,
                                        cost.ctypes.data, C.byref(in_place)))
        return cost, bool(in_place.value)

    def debug_scene_records(self, which):
        """One device record array of the built scene as it lies on the device (pt_debug_scene_records): `which` is a key of SCENE_RECORDS."""
        idx, dtype = SCENE_RECORDS[which]
        n = C.c_size_t()
        _check(self._L.pt_debug_scene_records(self._h, idx, None, 0, C.byref(n)))
        out = np.empty(n.value // 4, dtype)
        _check(self._L.pt_debug_scene_records(self._h, idx, out.ctypes.data, out.nbytes, C.byref(n)))
        return out

    # --- reprojection across moved geometry with bilinear taps (include/pt_motion_bilinear.h) ------
    def reproject_frame_moved_bilinear(self, max_history=64, depth_tol=0.02, normal_tol=0.9, snap=1 / 64, all_materials=False, albedo_floor=0.0):
        """reproject_frame_moved that blends the qualifying old pixels around the point a surface point projected to at the mark
        (pt_reproject_frame_moved_bilinear) where reproject_frame_moved copies the nearest one: a primitive that moves by a fraction of a pixel
        per step keeps its history in place.  The mark and the caller contract are reproject_frame_moved's, snap and albedo_floor
        reproject_frame_bilinear's.  Returns (kept, blended); the mark is spent.  Counts become fractional."""
        rule = ReprojectBilinearRule(float(max_history), float(depth_tol), float(normal_tol), float(snap), float(albedo_floor),
                                     self.REPROJECT_ALL_MATERIALS if all_materials else 0)
        n, nb = C.c_int64(0), C.c_int64(0)
        _check(self._L.pt_reproject_frame_moved_bilinear(self._h, C.byref(rule), C.byref(n), C.byref(nb)))
        return n.value, nb.value

    # --- history validation (include/pt_validate.h) -------------------------------------------------
    # defaults of validate_rule: the float32 model on the oracle's frames at 160 x 90 (tests/test_validate_abi.py), 64 frames,
    # one jump, 4 calls of 4 frames, clamped RMSE against 256 frames.  Light slid by 0.5 (M2): reproject only 0.0894, validated 0.0593 with
    # z = (3, 5) and 0.0610 with (2, 4), reset 0.1443; M1 pose 0 -> 8 (light fixed): 0.0418 / 0.0414 / 0.0419 / 0.1458.  Radius 2 gave 0.0600
    # on the light jump against 0.0593 for radius 3.
    VALIDATE_RADIUS = 3
    VALIDATE_Z = (3.0, 5.0)
    VALIDATE_NORMAL_TOL = 0.9

    def validate_rule(self, radius=None, z_lo=None, z_hi=None, normal_tol=None):
        """the pt_validate_rule of these arguments; None takes the defaults above"""
        return ValidateRule(int(self.VALIDATE_RADIUS if radius is None else radius), float(self.VALIDATE_Z[0] if z_lo is None else z_lo),
                            float(self.VALIDATE_Z[1] if z_hi is None else z_hi), float(self.VALIDATE_NORMAL_TOL if normal_tol is None else normal_tol))

    def history_hold(self):
        """Move FRAME and T of the current image aside and zero both (pt_history_hold): render the new frames next, with record_moments on, then
        history_merge.  After an upload that moves no surface (materials, textures) nothing is needed before the hold; a camera or geometry move
        goes through reproject_frame / motion_mark + reproject_frame_moved first."""
        _check(self._L.pt_history_hold(self._h))

    def history_merge(self, rule=None, want_kappa=False):
        """Add the held history back, scaled down per pixel where the new frames contradict it (pt_history_merge).  Returns how many pixels with
        a history had it reduced, or (that count, kappa as (H, W) float32 in FRAME order) with want_kappa.  The hold is spent."""
        rule = self.validate_rule() if rule is None else rule
        n = C.c_int64(0)
        kappa = np.zeros((self.H, self.W), dtype=np.float32) if want_kappa else None
        _check(self._L.pt_history_merge(self._h, C.byref(rule), kappa.ctypes.data if want_kappa else None, C.byref(n)))
        return (n.value, kappa) if want_kappa else n.value

    # --- outlier rejection (include/pt_despeckle.h) -------------------------------------------------
    # defaults of despeckle_rule: the float32 model on the oracle's frames at 160 x 90 (tests/test_despeckle_abi.py), whole-image
    # unclamped RMSE of the mean against 256 frames.  The best point of the grid radius {1, 2, 3} x sigmas {2, 3, 4} x own_z {3, +inf} on C3 at 4
    # frames: despeckled / raw = 0.884 (0.898 with own_z = 3); at 16 frames own_z = 3 is the better setting (0.947 against 0.997) and from there
    # on the one to pass.  min_taps, normal_tol and min_lum were held at the values below throughout.
    DESPECKLE_RADIUS = 1
    DESPECKLE_SIGMAS = 2.0
    DESPECKLE_MIN_TAPS = 4
    DESPECKLE_OWN_Z = float("inf")
    DESPECKLE_NORMAL_TOL = 0.9
    DESPECKLE_MIN_LUM = 0.0

    def despeckle_rule(self, radius=None, sigmas=None, min_taps=None, own_z=None, normal_tol=None, min_lum=None):
        """the pt_despeckle_rule of these arguments; None takes the defaults above"""
        return DespeckleRule(int(self.DESPECKLE_RADIUS if radius is None else radius), float(self.DESPECKLE_SIGMAS if sigmas is None else sigmas),
                             int(self.DESPECKLE_MIN_TAPS if min_taps is None else min_taps), float(self.DESPECKLE_OWN_Z if own_z is None else own_z),
                             float(self.DESPECKLE_NORMAL_TOL if normal_tol is None else normal_tol), float(self.DESPECKLE_MIN_LUM if min_lum is None else min_lum))

    def despeckle(self, rule=None, want_scale=False):
        """The current image with its firefly pixels pulled back to the ceiling of their surface neighbourhood (pt_despeckle), read only: FRAME
        and T stay as they are.  Returns (rgba as (H, W, 4) float32: the clamped mean and FRAME.a, the count of the pixels clamped), and with
        want_scale the factor per pixel as (H, W) float32 behind them."""
        rule = self.despeckle_rule() if rule is None else rule
        n = C.c_int64(0)
        out = np.zeros((self.H, self.W, 4), dtype=np.float32)
        scale = np.zeros((self.H, self.W), dtype=np.float32) if want_scale else None
        _check(self._L.pt_despeckle(self._h, C.byref(rule), out.ctypes.data, scale.ctypes.data if want_scale else None, C.byref(n)))
        return (out, n.value, scale) if want_scale else (out, n.value)

    def despeckle_frame(self, rule=None, want_scale=False):
        """The same rule stored: FRAME (and T, when allocated) of the current image are replaced (pt_despeckle_frame), so that every later call
        — filters, steering, fill, reprojections, hold / merge, display — sees the clamped image.  Irreversible, and it removes energy
        (include/pt_despeckle.h).  Returns the count of the pixels clamped, or (that count, the factor per pixel) with want_scale."""
        rule = self.despeckle_rule() if rule is None else rule
        n = C.c_int64(0)
        scale = np.zeros((self.H, self.W), dtype=np.float32) if want_scale else None
        _check(self._L.pt_despeckle_frame(self._h, C.byref(rule), scale.ctypes.data if want_scale else None, C.byref(n)))
        return (n.value, scale) if want_scale else n.value

    # --- the display image: metered exposure, tone curve, sRGB transfer (include/pt_tonemap.h) -------
    # defaults of tonemap_rule: PROVISIONAL — common choices (the ACES fit, sRGB, a key of 0.18, the 10 % .. 95 % ranks metered), not tuned on this
    # project's workloads
    TONEMAP_DEFAULTS = dict(curve=2, transfer=1, exposure=0.0, key=0.18, lo_pct=0.10, hi_pct=0.95, min_exposure=2.0 ** -10, max_exposure=2.0 ** 10,
                            white=4.0, adapt=1.0)

    def tonemap_rule(self, **kw):
        """the pt_tonemap_rule of these fields; a field not given takes TONEMAP_DEFAULTS'"""
        unknown = set(kw) - set(self.TONEMAP_DEFAULTS)
        assert not unknown, f"no such field of pt_tonemap_rule: {sorted(unknown)}"
        v = dict(self.TONEMAP_DEFAULTS, **kw)
        return TonemapRule(int(v["curve"]), int(v["transfer"]), float(v["exposure"]), float(v["key"]), float(v["lo_pct"]), float(v["hi_pct"]),
                           float(v["min_exposure"]), float(v["max_exposure"]), float(v["white"]), float(v["adapt"]))

    def _tonemap_image(self, image):
        if image is None:
            return None
        image = np.ascontiguousarray(image, dtype=np.float32)
        assert image.size == self.W * self.H * 4, "an (H, W, 4) float32 image in FRAME order: rgb a mean, a = FRAME.a"
        return image

    def tonemap(self, image=None, prev_exposure=0.0, rule=None, want_hist=False):
        """The display image (pt_tonemap) of the current FRAME, or of `image` — (H, W, 4) float32 in FRAME order, rgb a mean and a = FRAME.a:
        what denoise*, denoise_guided*, despeckle and fill_frame return.  Exposed (metered from the luminance histogram, damped towards
        prev_exposure by rule.adapt, or rule.exposure), tone-mapped and encoded.  Read only.  Returns ((H, W, 3) uint8, top row first, the
        exposure applied — feed it back as prev_exposure of the next step), and with want_hist the histogram (512 uint32) behind them."""
        rule = self.tonemap_rule() if rule is None else rule
        image = self._tonemap_image(image)
        out = np.zeros((self.H, self.W, 3), dtype=np.uint8)
        e = C.c_float(0.0)
        hist = np.zeros(TONEMAP_BINS, dtype=np.uint32) if want_hist else None
        _check(self._L.pt_tonemap(self._h, C.byref(rule), None if image is None else image.ctypes.data, float(prev_exposure), out.ctypes.data,
                                  C.byref(e), hist.ctypes.data if want_hist else None))
        return (out, e.value, hist) if want_hist else (out, e.value)

    def tonemap_png(self, path, image=None, prev_exposure=0.0, rule=None):
        """tonemap's image written as an 8-bit RGB PNG (pt_tonemap_save_png); returns the exposure applied"""
        rule = self.tonemap_rule() if rule is None else rule
        image = self._tonemap_image(image)
        e = C.c_float(0.0)
        _check(self._L.pt_tonemap_save_png(self._h, C.byref(rule), None if image is None else image.ctypes.data, float(prev_exposure),
                                           os.fsencode(path), C.byref(e)))
        return e.value

    # --- HDR glare ahead of the tone curve, and the display image of a device-resident image (include/pt_bloom.h) -------
    bloom_rule = staticmethod(bloom_rule)

    def _bloom_source(self, image):
        """(PT_BLOOM_SRC_*, the host image or None) of an `image` argument: None is FRAME, the string "filtered" the image the last filter call
        left on the device, an array a host image"""
        if image is None:
            return BLOOM_SRC_FRAME, None
        if isinstance(image, str):
            assert image == "filtered", 'a source by name is "filtered"'
            return BLOOM_SRC_FILTERED, None
        return BLOOM_SRC_HOST, self._tonemap_image(image)

    def bloom(self, image=None, exposure=1.0, bloom=None):
        """The float image with its glare (pt_bloom): (H, W, 4) float32, rgb a mean and a the source's a.  image: None (the current FRAME),
        "filtered" (what the last denoise* / denoise_guided* / read_display_denoised* call left on the device) or an (H, W, 4) float32 image in
        FRAME order.  exposure only scales bloom.threshold.  Read only."""
        bloom = bloom_rule() if bloom is None else bloom
        source, image = self._bloom_source(image)
        out = np.zeros((self.H, self.W, 4), dtype=np.float32)
        _check(self._L.pt_bloom(self._h, C.byref(bloom), source, None if image is None else image.ctypes.data, float(exposure), out.ctypes.data))
        return out

    def tonemap_bloom(self, image=None, prev_exposure=0.0, rule=None, bloom=None, want_hist=False):
        """tonemap with the glare between the metering and the curve (pt_tonemap_bloom), all on the device; `image` as bloom's.  The exposure
        and the histogram are tonemap's of the same source whatever the bloom rule.  Returns what tonemap returns."""
        rule = self.tonemap_rule() if rule is None else rule
        bloom = bloom_rule() if bloom is None else bloom
        source, image = self._bloom_source(image)
        out = np.zeros((self.H, self.W, 3), dtype=np.uint8)
        e = C.c_float(0.0)
        hist = np.zeros(TONEMAP_BINS, dtype=np.uint32) if want_hist else None
        _check(self._L.pt_tonemap_bloom(self._h, C.byref(rule), C.byref(bloom), source, None if image is None else image.ctypes.data, float(prev_exposure),
                                        out.ctypes.data, C.byref(e), hist.ctypes.data if want_hist else None))
        return (out, e.value, hist) if want_hist else (out, e.value)

    def tonemap_bloom_save_png(self, path, image=None, prev_exposure=0.0, rule=None, bloom=None):
        """tonemap_bloom's image written as an 8-bit RGB PNG (pt_tonemap_bloom_save_png); returns the exposure applied"""
        rule = self.tonemap_rule() if rule is None else rule
        bloom = bloom_rule() if bloom is None else bloom
        source, image = self._bloom_source(image)
        e = C.c_float(0.0)
        _check(self._L.pt_tonemap_bloom_save_png(self._h, C.byref(rule), C.byref(bloom), source, None if image is None else image.ctypes.data,
                                                 float(prev_exposure), os.fsencode(path), C.byref(e)))
        return e.value

    # --- luminance moments and the variance-guided filter (include/pt_guided.h) ---------------------
    # defaults of denoise_guided / read_display_denoised_guided: sigma_lum and min_frames from scripts/guided_quality.py's grid on C3 and C6
    # at 1080p (profiles/r11_guided_quality.txt); the geometric sigmas are DENOISE_SIGMAS'
    GUIDED_SIGMA_LUM = 2.0
    GUIDED_MIN_FRAMES = 4
    # albedo_floor=None on the calls below and on reproject_frame makes the plain call; a number (ALBEDO_FLOOR is the module's default for it) makes
    # the albedo-demodulated one of include/pt_demod.h, where sigma_albedo=float('inf') is the natural setting

    def record_moments(self, on=True):
        """Record T = (sY, sYY, n, 0), the per-pixel luminance moments, for every frame rendered from now on (pt_record_moments)"""
        _check(self._L.pt_record_moments(self._h, 1 if on else 0))

    def read_moments(self):
        """T of the current image (pt_read_moments): (H, W, 4) float32 (sY, sYY, n, 0), FRAME order; zeros when never recorded"""
        out = np.zeros((self.H, self.W, 4), dtype=np.float32)
        _check(self._L.pt_read_moments(self._h, out.ctypes.data))
        return out

    def write_moments(self, moments):
        """replace T of the current image (pt_write_moments); pt_write_frame zeroes T, so restore FRAME first"""
        m = np.ascontiguousarray(moments, dtype=np.float32)
        assert m.size == self.W * self.H * 4
        _check(self._L.pt_write_moments(self._h, m.ctypes.data))

    def _guided_args(self, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames):
        g = self._sigmas(None, sigma_normal, sigma_depth, sigma_albedo)
        g[0] = float(self.GUIDED_SIGMA_LUM if sigma_lum is None else sigma_lum)
        return g + [int(self.GUIDED_MIN_FRAMES if min_frames is None else min_frames)]

    def denoise_guided(self, iterations=5, sigma_lum=None, sigma_normal=None, sigma_depth=None, sigma_albedo=None, min_frames=None, albedo_floor=None,
                       fill=False, through=None):
        """the variance-guided filter over FRAME.rgb / FRAME.a, steered by T (pt_denoise_guided): (H, W, 4) float32, rgb = filtered mean,
        a = FRAME.a.  Needs moments (record_moments before rendering, or write_moments).  None takes the defaults above.
        albedo_floor: a number filters the illumination mean / albedo instead (pt_denoise_guided_demod).
        fill: reconstruct the pixels nothing was rendered into first (pt_denoise_guided_filled, include/pt_fill.h): after render_interleaved.
        through: with fill, a through_rule(): fill and filter on the seen-through records (pt_denoise_guided_through, include/pt_through.h)."""
        out = np.zeros((self.H, self.W, 4), dtype=np.float32)
        g = self._guided_args(sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames)
        if through is not None:
            if not fill:
                raise ValueError("through= needs fill=True")
            _check(self._L.pt_denoise_guided_through(self._h, C.byref(through), int(iterations), *g, 0.0 if albedo_floor is None else float(albedo_floor),
                                                     out.ctypes.data))
        elif fill:
            _check(self._L.pt_denoise_guided_filled(self._h, int(iterations), *g, 0.0 if albedo_floor is None else float(albedo_floor), out.ctypes.data))
        elif albedo_floor is None:
            _check(self._L.pt_denoise_guided(self._h, int(iterations), *g, out.ctypes.data))
        else:
            _check(self._L.pt_denoise_guided_demod(self._h, int(iterations), *g, float(albedo_floor), out.ctypes.data))
        return out

    def read_display_denoised_guided(self, iterations=5, sigma_lum=None, sigma_normal=None, sigma_depth=None, sigma_albedo=None, min_frames=None,
                                     java_bytes=True, albedo_floor=None, fill=False, through=None):
        """denoise_guided()'s image converted to 8 bits as read_display converts a mean: (H, W, 3) uint8, top row first"""
        out = np.zeros((self.H, self.W, 3), dtype=np.uint8)
        g = self._guided_args(sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames)
        jb = 1 if java_bytes else 0
        if through is not None:
            if not fill:
                raise ValueError("through= needs fill=True")
            _check(self._L.pt_read_display_denoised_guided_through(self._h, C.byref(through), int(iterations), *g,
                                                                   0.0 if albedo_floor is None else float(albedo_floor), jb, out.ctypes.data))
        elif fill:
            _check(self._L.pt_read_display_denoised_guided_filled(self._h, int(iterations), *g, 0.0 if albedo_floor is None else float(albedo_floor), jb,
                                                                  out.ctypes.data))
        elif albedo_floor is None:
            _check(self._L.pt_read_display_denoised_guided(self._h, int(iterations), *g, jb, out.ctypes.data))
        else:
            _check(self._L.pt_read_display_denoised_guided_demod(self._h, int(iterations), *g, float(albedo_floor), jb, out.ctypes.data))
        return out

    # --- interleaved rendering (include/pt_fill.h) ------------------------------------------------------
    def render_interleaved(self, first_frame, seeds, stride=2, phase_x=0, phase_y=0):
        """Frames first_frame.. (one per seed) for the pixels x % stride == phase_x, y % stride == phase_y (FRAME order, row 0 = bottom):
        render_mask with that mask, built on the device (pt_render_interleaved).  Returns how many pixels were rendered.  Show the image with
        denoise_guided(fill=True) / read_display_denoised_guided(fill=True)."""
        s = np.ascontiguousarray(seeds, dtype=np.int32)
        n = C.c_int64(0)
        _check(self._L.pt_render_interleaved(self._h, int(first_frame), int(s.size), s.ctypes.data, int(stride), int(phase_x), int(phase_y), C.byref(n)))
        return n.value

    def fill_frame(self, sigma_normal=None, sigma_depth=None, sigma_albedo=None, albedo_floor=None, through=None):
        """FRAME with every pixel nothing was rendered into reconstructed from the rendered neighbours of its surface (pt_fill_frame):
        ((H, W, 4) float32 in FRAME's layout, how many pixels were filled).  FRAME is not modified.  albedo_floor: a number interpolates
        the illumination and gives a filled pixel its own albedo."""
        out = np.zeros((self.H, self.W, 4), dtype=np.float32)
        g = self._sigmas(None, sigma_normal, sigma_depth, sigma_albedo)
        n = C.c_int64(0)
        fl = 0.0 if albedo_floor is None else float(albedo_floor)
        if through is not None:                                   # a through_rule(): the seen-through records in place of the first-hit ones
            _check(self._L.pt_fill_frame_through(self._h, C.byref(through), g[1], g[2], g[3], fl, out.ctypes.data, C.byref(n)))
        else:
            _check(self._L.pt_fill_frame(self._h, g[1], g[2], g[3], fl, out.ctypes.data, C.byref(n)))
        return out, n.value

    # --- seen-through feature records (include/pt_through.h) --------------------------------------------
    THROUGH_REFLECT, THROUGH_TRANSMIT, THROUGH_KEY = 1, 2, 1
    # defaults of through_rule: the variant of scripts/through_quality.py that is best on the filled metal pixels of C3 and C6 at 1080p among those
    # that lose on no scene's overall clamped error at 16 lattice frames (profiles/r15_through_quality.txt): reflection only, at
    # 0.8, without the key.  Both lobes at 0.5 lose on C3 and C6.  No call takes a rule unless it is given one (through=None).
    THROUGH_DEPTH = 4
    THROUGH_MIN_WEIGHT = 0.8
    THROUGH_LOBES = 1
    THROUGH_USE_KEY = False

    def through_rule(self, max_depth=None, min_weight=None, lobes=None, key=None):
        """the pt_through_rule of these arguments; None takes the defaults above"""
        key = self.THROUGH_USE_KEY if key is None else key
        return ThroughRule(int(self.THROUGH_DEPTH if max_depth is None else max_depth), float(self.THROUGH_MIN_WEIGHT if min_weight is None else min_weight),
                           int(self.THROUGH_LOBES if lobes is None else lobes), self.THROUGH_KEY if key else 0)

    def read_features_through(self, rule=None):
        """the feature records followed through mirrors and glass (pt_read_features_through): (H, W, 16) float32 in read_features' layout, with
        the chain's length L in place of t, tint * Kd in place of Kd, the surface word in place of the material and k in slot 14"""
        rule = self.through_rule() if rule is None else rule
        out = np.zeros((self.H, self.W, 16), dtype=np.float32)
        _check(self._L.pt_read_features_through(self._h, C.byref(rule), out.ctypes.data))
        return out

    def read_through_rays(self, rule=None):
        """(H, W, 8) float32: (O, t, D, k as int32 bits) of the segment that found each pixel's recorded surface (pt_read_through_rays)"""
        rule = self.through_rule() if rule is None else rule
        out = np.zeros((self.H, self.W, 8), dtype=np.float32)
        _check(self._L.pt_read_through_rays(self._h, C.byref(rule), out.ctypes.data))
        return out

    # --- adaptive sampling steered by the guided filter (include/pt_steer.h) ---------------------------
    def render_mask(self, first_frame, seeds, mask):
        """Frames first_frame.. (one per seed) for the pixels where mask != 0 ((H, W), FRAME order, row 0 = bottom) and not under the mouse
        overlay (pt_render_mask); FRAME and T as render_adaptive updates them.  Returns how many pixels were rendered."""
        s = np.ascontiguousarray(seeds, dtype=np.int32)
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        assert m.size == self.W * self.H
        n = C.c_int64(0)
        _check(self._L.pt_render_mask(self._h, int(first_frame), int(s.size), s.ctypes.data, m.ctypes.data, C.byref(n)))
        return n.value

    def guided_rule(self, rel_err, abs_err=0.0, iterations=5, sigma_lum=None, sigma_normal=None, sigma_depth=None, sigma_albedo=None, min_frames=None,
                    max_frames=0):
        """the pt_guided_rule of these arguments; None takes denoise_guided's defaults"""
        sl, sn, sd, sa, mf = self._guided_args(sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames)
        return GuidedRule(int(iterations), sl, sn, sd, sa, mf, float(rel_err), float(abs_err), int(max_frames))

    def select_guided(self, rel_err, abs_err=0.0, iterations=5, sigma_lum=None, sigma_normal=None, sigma_depth=None, sigma_albedo=None, min_frames=None,
                      max_frames=0, albedo_floor=None):
        """The pixels the guided filter still finds uncertain (pt_select_guided): (H, W) bool, FRAME order.  FRAME and T are not modified.
        albedo_floor: a number asks the demodulated filter (pt_select_guided_demod)."""
        out = np.zeros((self.H, self.W), dtype=np.uint8)
        rule = self.guided_rule(rel_err, abs_err, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames, max_frames)
        n = C.c_int64(0)
        if albedo_floor is None:
            _check(self._L.pt_select_guided(self._h, C.byref(rule), out.ctypes.data, C.byref(n)))
        else:
            _check(self._L.pt_select_guided_demod(self._h, C.byref(rule), float(albedo_floor), out.ctypes.data, C.byref(n)))
        return out.astype(bool)

    def render_adaptive_guided(self, first_frame, seeds, rel_err, abs_err=0.0, iterations=5, sigma_lum=None, sigma_normal=None, sigma_depth=None,
                               sigma_albedo=None, min_frames=None, max_frames=0, albedo_floor=None):
        """select_guided, then render_mask on its selection (pt_render_adaptive_guided, or pt_render_adaptive_guided_demod when albedo_floor is
        a number); returns how many pixels were rendered"""
        s = np.ascontiguousarray(seeds, dtype=np.int32)
        rule = self.guided_rule(rel_err, abs_err, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames, max_frames)
        n = C.c_int64(0)
        if albedo_floor is None:
            _check(self._L.pt_render_adaptive_guided(self._h, int(first_frame), int(s.size), s.ctypes.data, C.byref(rule), C.byref(n)))
        else:
            _check(self._L.pt_render_adaptive_guided_demod(self._h, int(first_frame), int(s.size), s.ctypes.data, C.byref(rule), float(albedo_floor), C.byref(n)))
        return n.value

    def screenshot(self, path, frame_count, java_bytes=True):
        """functions.screenshot(fileName) (dispatch.java:804-851): the display image as a PNG file, written by the library (pt_save_png)"""
        _check(self._L.pt_save_png(self._h, int(frame_count), 1 if java_bytes else 0, str(path).encode()))

    def frame_device(self):
        p, n = C.c_void_p(), C.c_size_t()
        _check(self._L.pt_frame_device(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def unshard(self, gathered_ptr, full_ptr):
        _check(self._L.pt_unshard(self._h, C.c_void_p(gathered_ptr), C.c_void_p(full_ptr)))

    def set_stream(self, hip_stream):
        _check(self._L.pt_set_stream(self._h, C.c_void_p(hip_stream)))

    def set_option(self, name, value):
        _check(self._L.pt_set_option(self._h, OPTIONS[name], int(value)))

    # --- statistics ---------------------------------------------------------------------------
    def counters(self):
        out = np.zeros(len(COUNTERS), dtype=np.uint64)
        _check(self._L.pt_get_counters(self._h, out.ctypes.data, len(COUNTERS)))
        return dict(zip(COUNTERS, [int(x) for x in out]))

    def reset_counters(self):
        _check(self._L.pt_reset_counters(self._h))

    def set_timing(self, on):
        _check(self._L.pt_set_timing(self._h, 1 if on else 0))

    def kernel_time(self, name):
        n, ms = C.c_int64(), C.c_double()
        _check(self._L.pt_kernel_time(self._h, KERNELS[name], C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def kernel_time_median(self, name):
        ms = C.c_double()
        _check(self._L.pt_kernel_time_median(self._h, KERNELS[name], C.byref(ms)))
        return ms.value

    # --- parity probes --------------------------------------------------------------------------
    def debug_math(self, fn, x, y=None):
        # rng_state / rng_result / rng_random: one NextRandom / random() call of frag.glsl:686-694, the uint32 state travels as float bits
        names = {"sin": 0, "cos": 1, "log": 2, "exp": 3, "atan2": 4, "asin": 5, "rng_state": 6, "rng_result": 7, "rng_random": 8, "unorm8": 9}
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        yp = None if y is None else np.ascontiguousarray(y, dtype=np.float32).ctypes.data
        _check(self._L.pt_debug_math(self._h, names[fn], x.ctypes.data, yp, out.ctypes.data, x.size))
        return out

    def debug_intersect(self, o, d):
        o = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
        out = np.empty((o.shape[0], 4), dtype=np.float32)
        _check(self._L.pt_debug_intersect(self._h, o.ctypes.data, d.ctypes.data, out.ctypes.data, o.shape[0]))
        return out[:, :3].copy(), out[:, 3].copy().view(np.int32)
