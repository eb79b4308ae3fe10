"""A float32 model of adaptive sampling (include/pt_adaptive.h): the selection rule and the FRAME / T updates of pt_render_adaptive and
pt_render_batch, replayed from the colour every frame adds (not a test module: the helpers of tests/test_adaptive_abi.py,
tests/test_gpu_adaptive.py and tests/test_gpu_adaptive_sizes.py)."""
import numpy as np


def select(T, rel_err, abs_err, min_frames, max_frames, overlay=None):
    """the selection rule of include/pt_adaptive.h over T = (..., 4) float32 (sY, sYY, n, 0), evaluated in float32 in the header's order"""
    T = np.asarray(T, np.float32)
    sY, sYY, n = T[..., 0], T[..., 1], T[..., 2]
    with np.errstate(all="ignore"):
        mean = sY / n
        var = (sYY - sY * mean) / (n - np.float32(1.0))
        err2 = var / n
        tol = np.fmax(np.float32(rel_err) * np.abs(mean), np.float32(abs_err))
        act = err2 > tol * tol
    act = act | (n < np.float32(min_frames))
    if max_frames > 0:
        act = act & ~(n >= np.float32(max_frames))
    if overlay is not None:
        act = act & ~overlay
    return act


def rel_ratio(T):
    """per pixel sqrt(err2) / |mean| in float64 from the float32 err2 and mean of the rule: the rel_err at which the pixel changes side"""
    T = np.asarray(T, np.float32)
    sY, sYY, n = T[..., 0], T[..., 1], T[..., 2]
    with np.errstate(all="ignore"):
        mean = sY / n
        err2 = ((sYY - sY * mean) / (n - np.float32(1.0))) / n
        return np.sqrt(err2.astype(np.float64)) / np.abs(mean.astype(np.float64)), np.sqrt(err2.astype(np.float64))


def tolerance_for_count(T, k, min_frames=2):
    """(rel_err, abs_err) under which exactly k pixels of T are active, confirmed with the float32 select and nudged by single ulps where the
    float64 midpoint lands on the wrong side of a pixel.  First rel_err from the ranking of sqrt(err2)/|mean| with abs_err 0; where pixels tie
    there (a pixel with one non-black frame has the ratio 1 whatever its colour), abs_err from the ranking of sqrt(err2) with rel_err 0.
    None when neither reaches k."""
    for which in (0, 1):
        r = rel_ratio(T)[which].ravel()
        r = np.sort(r[np.isfinite(r)])[::-1]                  # largest first: the k noisiest pixels are the active ones
        if not 0 < k < r.size:
            continue

        def count(v):
            return int(select(T, v, 0.0, min_frames, 0).sum()) if which == 0 else int(select(T, 0.0, v, min_frames, 0).sum())
        v = np.float32(0.5 * (r[k - 1] + r[k]))
        got = count(v)
        for _ in range(64):
            if got == k:
                return (float(v), 0.0) if which == 0 else (0.0, float(v))
            nxt = np.nextafter(v, np.float32(np.inf) if got > k else np.float32(0))     # a larger tolerance selects fewer pixels
            g2 = count(nxt)
            if g2 != k and (g2 > k) != (got > k):
                break                                         # the count jumps over k between two adjacent floats
            v, got = nxt, g2
    return None


class Model:
    """FRAME and T = (sY, sYY, n, 0) of one image, as pt_render_adaptive / pt_render_batch update them; cols[f - 1] = the (H, W, 3) float32
    rgb that frame f adds to each pixel"""

    def __init__(self, cols):
        self.cols = cols
        H, W = cols[0].shape[:2]
        self.F = np.zeros((H, W, 4), np.float32)
        self.T = np.zeros((H, W, 4), np.float32)

    def _add(self, f, m):
        c = self.cols[f - 1]
        if f == 1:
            self.F[m] = np.concatenate([c[m], np.ones((int(m.sum()), 1), np.float32)], axis=1)
        else:
            self.F[m, :3] = self.F[m, :3] + c[m]
            self.F[m, 3] = self.F[m, 3] + np.float32(1.0)

    def adaptive(self, first, n, rel_err, abs_err=0.0, min_frames=4, max_frames=0):
        act = select(self.T, rel_err, abs_err, min_frames, max_frames)
        self.frames(first, n, act)
        return act

    def frames(self, first, n, act):
        """frames first .. first+n-1 on the pixels of `act`, into FRAME and T (an adaptive call whose selection is given)"""
        for f in range(first, first + n):
            self._add(f, act)
            c = self.cols[f - 1][act]
            Y = (np.float32(0.2126) * c[:, 0] + np.float32(0.7152) * c[:, 1]) + np.float32(0.0722) * c[:, 2]
            self.T[act, 0] = self.T[act, 0] + Y
            self.T[act, 1] = self.T[act, 1] + Y * Y
            self.T[act, 2] = self.T[act, 2] + np.float32(1.0)

    def uniform(self, first, n):
        for f in range(first, first + n):
            self._add(f, np.ones(self.F.shape[:2], bool))

    def reset_stats(self):
        self.T[:] = 0
