"""A float32 model of the selection rule of include/pt_steer.h, built on the guided filter's model (tests/_guided_model.py) and the own-moment rule
of include/pt_adaptive.h (tests/_adaptive_model.py) (not a test module: the helpers of tests/test_steer_abi.py and tests/test_gpu_steer.py)."""
import numpy as np

from _adaptive_model import select
from _denoise_model import classify
from _guided_model import INF32, denoise_guided, lum, variance


def filtered(frame, feat, T, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames):
    """(c_K, v_K): the filtered mean (H, W, 3) and its carried variance (H, W); K = 0 takes the mean and v_0 = s2 / A straight from variance()"""
    frame = np.asarray(frame, np.float32)
    if iterations == 0:
        c, _ = classify(frame, feat)
        return c, variance(frame, feat, T, min_frames)
    out, v = denoise_guided(frame, feat, T, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames, return_var=True)
    return out[..., :3], v


def select_guided(frame, feat, T, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames, rel_err, abs_err=0.0, max_frames=0,
                  overlay=None, detail=False):
    """the rule's (H, W) bool mask; detail: also a dict of the step that decided each pixel ("step": 1 .. 5) and step 5's v_K and tol^2"""
    frame = np.asarray(frame, np.float32)
    T = np.asarray(T, np.float32)
    _, cls = classify(frame, feat)
    n = T[..., 2]
    c, v = filtered(frame, feat, T, iterations, sigma_lum, sigma_normal, sigma_depth, sigma_albedo, min_frames)
    with np.errstate(all="ignore"):
        tol = np.fmax(np.float32(rel_err) * np.abs(lum(c)), np.float32(abs_err)).astype(np.float32)
        tol2 = (tol * tol).astype(np.float32)
        guided = (v == INF32) | (v > tol2)
    own = select(T, rel_err, abs_err, min_frames, 0)                     # steps 3 and 4 for the invalid pixels
    act = np.where(cls == 0, own, guided | (n < np.float32(min_frames)))
    step = np.where(cls == 0, 4, 5)
    step = np.where(n < np.float32(min_frames), 3, step)
    if max_frames > 0:
        cap = n >= np.float32(max_frames)
        act = act & ~cap
        step = np.where(cap, 2, step)
    if overlay is not None:
        act = act & ~overlay
        step = np.where(overlay, 1, step)
    if detail:
        return act, {"step": step, "v": v, "tol2": tol2}
    return act
