"""A float32 numpy model of the a-trous denoiser of include/pt_denoise.h, written from the header's text (not a test module: the helpers of
tests/test_denoise_abi.py and tests/test_gpu_denoise.py)."""
import numpy as np

F32_MAX = np.float32(np.finfo(np.float32).max)
H5 = np.array([1, 4, 6, 4, 1], np.float32) / np.float32(16)


def _inv(num, sigma):
    """num / sigma^2 in float32, clamped to the largest float so that a zero difference never meets an infinity (sigma tiny)"""
    s = np.float32(sigma)
    with np.errstate(all="ignore"):
        return np.minimum(np.float32(num) / (s * s), F32_MAX)


def classify(frame, feat):
    """(c, cls): the filter's input (mean, or raw rgb where FRAME.a <= 0) and the class of every pixel: 0 invalid, 1 hit, 2 miss"""
    frame = np.asarray(frame, np.float32)
    feat = np.asarray(feat, np.float32)
    a = frame[..., 3]
    with np.errstate(all="ignore"):
        mean = frame[..., :3] / a[..., None]
    hit = np.ascontiguousarray(feat[..., 7]).view(np.int32) >= 0
    valid = (a > 0) & np.isfinite(mean).all(-1) & np.isfinite(feat[..., 0:7]).all(-1)
    c = np.where((a > 0)[..., None], mean, frame[..., :3]).astype(np.float32)
    cls = np.where(valid, np.where(hit, 1, 2), 0)
    return c, cls


def denoise(frame, feat, iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo):
    """(H, W, 4) float32: rgb = the denoised mean, a = FRAME.a"""
    frame = np.asarray(frame, np.float32)
    feat = np.asarray(feat, np.float32)
    H, W = frame.shape[:2]
    c, cls = classify(frame, feat)
    t, N, Kd = feat[..., 0], feat[..., 1:4], feat[..., 4:7]
    invN, invD, invA = _inv(1, sigma_normal), _inv(1, sigma_depth), _inv(1, sigma_albedo)
    yy, xx = np.mgrid[0:H, 0:W]
    hitp = cls == 1
    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            invC = _inv(4 ** i, sigma_color)
            num = np.zeros((H, W, 3), np.float32)
            den = np.zeros((H, W), np.float32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = yy + dy * s, xx + dx * s
                    inb = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    cq = c[qy, qx]
                    use = inb & (cls != 0) & (cls[qy, qx] == cls)
                    e = ((c - cq) ** 2).sum(-1, dtype=np.float32) * invC
                    dt = (t - t[qy, qx]) / t
                    g = ((N - N[qy, qx]) ** 2).sum(-1, dtype=np.float32) * invN + (dt * dt) * invD + ((Kd - Kd[qy, qx]) ** 2).sum(-1, dtype=np.float32) * invA
                    e = np.where(hitp, e + g, e).astype(np.float32)
                    w = (H5[dy + 2] * H5[dx + 2]) * np.exp(-e).astype(np.float32)
                    num += np.where(use[..., None], w[..., None] * cq, np.float32(0))
                    den += np.where(use, w, np.float32(0))
            c = np.where((cls != 0)[..., None], num / den[..., None], c).astype(np.float32)
    return np.concatenate([c, frame[..., 3:4]], axis=-1).astype(np.float32)


def features(H, W, t=1.0, normal=(0.0, 1.0, 0.0), albedo=(0.5, 0.5, 0.5), hit=0x1000000):
    """a synthetic feature image: every pixel the same record (hit code -1 makes it a miss)"""
    f = np.zeros((H, W, 16), np.float32)
    f[..., 0] = t
    f[..., 1:4] = normal
    f[..., 4:7] = albedo
    f[..., 7] = np.array([hit], np.int32).view(np.float32)[0]
    return f
