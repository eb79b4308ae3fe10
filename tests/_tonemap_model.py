"""The float32 numpy model of include/pt_tonemap.h, steps 1-5: what pt_tonemap must equal bit for bit.  Every array operation below is one
binary32 operation per element in the header's order (numpy contracts nothing); step 3 is Python's binary64 and exact integers.  A rule is
a dict of the struct's fields; T is the threshold table (pt_tonemap_srgb_thresholds, whose bracket property test_tonemap_abi.py checks)."""
import math

import numpy as np

f32 = np.float32
BINS = 512
RULE = dict(curve=2, transfer=1, exposure=0.0, key=0.18, lo_pct=0.10, hi_pct=0.95, min_exposure=2.0 ** -10, max_exposure=2.0 ** 10, white=4.0, adapt=1.0)


def rule(**kw):
    assert not set(kw) - set(RULE)
    return dict(RULE, **kw)


def from_frame(frame):
    """(c, A) of a FRAME image (rgb a running sum, a the count): three divisions per pixel"""
    frame = np.asarray(frame, dtype=f32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        return frame[:, :3] / frame[:, 3:4], frame[:, 3].copy()


def from_image(image):
    """(c, A) of an image in pt_denoise_guided's output convention: rgb is a mean already"""
    image = np.asarray(image, dtype=f32).reshape(-1, 4)
    return image[:, :3].copy(), image[:, 3].copy()


def luminance(c):
    with np.errstate(all="ignore"):
        return (f32(0.2126) * c[:, 0] + f32(0.7152) * c[:, 1]) + f32(0.0722) * c[:, 2]


def bin_of(l):
    """step 2's bin of every luminance (meaningful for the metered ones)"""
    return np.clip((np.ascontiguousarray(l, dtype=f32).view(np.uint32) >> 19).astype(np.int64) - 1776, 0, BINS - 1)


def bin_mid(b):
    return np.array([((int(b) + 1776) << 19) | (1 << 18)], dtype=np.uint32).view(f32)[0]


def metered(c, A):
    l = luminance(c)
    with np.errstate(all="ignore"):
        return (A > 0) & np.isfinite(l) & (l > 0)


def histogram(c, A):
    return np.bincount(bin_of(luminance(c))[metered(c, A)], minlength=BINS).astype(np.uint32)


def exposure(hist, r, prev=0.0):
    """step 3: the exposure as a float32"""
    if f32(r["exposure"]) > 0:
        return f32(r["exposure"])
    hist = [int(v) for v in hist]
    N = sum(hist)
    lo, hi = float(f32(r["min_exposure"])), float(f32(r["max_exposure"]))
    target = 1.0
    if N > 0:
        first = math.floor(float(f32(r["lo_pct"])) * N)
        end = N - math.floor((1.0 - float(f32(r["hi_pct"]))) * N)
        cum, K, S = 0, 0, 0.0
        for b in range(BINS):
            keep = max(0, min(cum + hist[b], end) - max(cum, first))
            K += keep
            S += float(keep) * float(bin_mid(b))
            cum += hist[b]
        if K > 0:
            target = float(f32(r["key"])) / (S / K)
    target = min(max(target, lo), hi)
    prev = float(f32(prev))
    e = prev + float(f32(r["adapt"])) * (target - prev) if prev > 0 else target
    return f32(e)


def codes(t, transfer, T):
    """step 5 of values t in [0, 1]"""
    t = np.asarray(t, dtype=f32)
    if transfer == 0:
        return np.floor(t * f32(255.0) + f32(0.5)).astype(np.uint8)
    return np.searchsorted(np.asarray(T, dtype=f32)[1:], t, side="right").astype(np.uint8)


def apply(c, A, e, r, T, W, H):
    """steps 4-5: the (H, W, 3) uint8 image, top row first"""
    one = f32(1.0)
    with np.errstate(all="ignore"):
        x = c * f32(e)
        x = np.where(np.isnan(x), f32(0), np.where(x < 0, f32(0), np.where(x > f32(65504.0), f32(65504.0), x))).astype(f32)
        if r["curve"] == 0:
            t = x
        elif r["curve"] == 1:
            w2 = f32(r["white"]) * f32(r["white"])
            t = (x * (one + x / w2)) / (one + x)
        else:
            t = (x * (f32(2.51) * x + f32(0.03))) / (x * (f32(2.43) * x + f32(0.59)) + f32(0.14))
        t = np.where(np.isnan(t), f32(0), np.where(t < 0, f32(0), np.where(t > one, one, t))).astype(f32)
        t = np.where((A > 0)[:, None], t, f32(0)).astype(f32)
    assert t.dtype == f32 and x.dtype == f32
    return codes(t, r["transfer"], T).reshape(H, W, 3)[::-1].copy()


def tonemap(c, A, r, T, W, H, prev=0.0):
    """(bytes, exposure, histogram) of pt_tonemap for (c, A) from from_frame or from_image"""
    hist = histogram(c, A)
    e = exposure(hist, r, prev)
    return apply(c, A, e, r, T, W, H), e, hist
