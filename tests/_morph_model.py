"""The rule of include/pt_morph.h in numpy binary32: per corner its entries in ascending target order, an entry whose weight compares equal to
zero skipped, every product rounded before every sum; composed with tests/_pose_model.py and tests/_skin_model.py (the morphed rest pose takes
the rest pose's place).  Also the two sums the rule is NOT (fused, and binary64 rounded once), so that a test can show the comparison tells them
apart, and the cases the CPU and GPU tests share.  A table here is a list of targets (corners int32[m], deltas float32[m, 6])."""
import numpy as np

import _pose_model as PM
import _skin_model as SM

f32 = np.float32


def _columns(corners):
    """the six float columns of binding 3 (as (n, 40)) that corner q = 3k + c owns: (rows, columns), shape (m, 6) each"""
    q = np.asarray(corners, np.int64).reshape(-1)
    k, c = q // 3, q % 3
    cols = np.concatenate([4 * c[:, None] + np.arange(3)[None, :], 12 + 4 * c[:, None] + np.arange(3)[None, :]], axis=1)
    return np.repeat(k[:, None], 6, axis=1), cols


def morph(rest, targets, weights):
    """rest: 40 floats per triangle -> the morphed rest pose.  One target after the other: a target names a corner at most once, so the order
    of a corner's sums is the ascending target order."""
    out = np.ascontiguousarray(rest, f32).reshape(-1, 40).copy()
    w = np.ascontiguousarray(weights, f32).reshape(-1)
    assert w.size == len(targets)
    with np.errstate(all="ignore"):
        for t, (corners, deltas) in enumerate(targets):
            if w[t] == 0.0 or len(corners) == 0:
                continue
            rows, cols = _columns(corners)
            p = (w[t] * np.ascontiguousarray(deltas, f32).reshape(-1, 6)).astype(f32)
            out[rows, cols] = (out[rows, cols] + p).astype(f32)
    return out.reshape(-1)


def morph_f64(rest, targets, weights):
    """what the rule is not: the sums in binary64, rounded once"""
    out = np.ascontiguousarray(rest, f32).reshape(-1, 40).astype(np.float64)
    w = np.ascontiguousarray(weights, f32).astype(np.float64)
    for t, (corners, deltas) in enumerate(targets):
        if w[t] == 0.0 or len(corners) == 0:
            continue
        rows, cols = _columns(corners)
        out[rows, cols] += w[t] * np.ascontiguousarray(deltas, f32).reshape(-1, 6).astype(np.float64)
    return out.astype(f32).reshape(-1)


def morph_fma(rest, targets, weights):
    """what the rule is not: v = fma(w, d, v), the chain a compiler contracts it to"""
    out = np.ascontiguousarray(rest, f32).reshape(-1, 40).copy()
    w = np.ascontiguousarray(weights, f32)
    for t, (corners, deltas) in enumerate(targets):
        if w[t] == 0.0 or len(corners) == 0:
            continue
        rows, cols = _columns(corners)
        d = np.ascontiguousarray(deltas, f32).reshape(-1, 6)
        for e in range(len(rows)):
            for j in range(6):
                out[rows[e, j], cols[e, j]] = PM._fma(w[t], d[e, j], out[rows[e, j], cols[e, j]])
    return out.reshape(-1)


def morph_pose(rest, targets, weights, tri_part, xforms):
    """pt_pose_triangles of a pose of pt_pose_create with a morph"""
    return PM.pose(morph(rest, targets, weights), tri_part, xforms)


def morph_skin(rest, targets, weights, bone, weight, xforms):
    """pt_pose_triangles of a pose of pt_skin_create with a morph"""
    return SM.skin(morph(rest, targets, weights), bone, weight, xforms)


def moved_corners(n_tris, tri_part=None, bone=None):
    """the corners the pose's rule moves, ascending: those that may carry entries"""
    if bone is not None:
        return np.nonzero(np.asarray(bone).reshape(-1, 4)[:, 0] >= 0)[0].astype(np.int32)
    return np.nonzero(np.repeat(np.asarray(tri_part).reshape(-1) >= 0, 3))[0].astype(np.int32)


def random_targets(allowed, n_affected, n_targets, seed=3, all_targets_corner=True, scale=0.3):
    """n_targets targets over n_affected corners drawn from `allowed`: rows of uneven length (every affected corner is named by at least one
    target, the first one by every target when all_targets_corner), the entries shuffled within each target.  -> (targets, affected ascending)"""
    rng = np.random.RandomState(seed)
    allowed = np.asarray(allowed, np.int32)
    n_affected = min(n_affected, allowed.size)
    affected = np.sort(rng.choice(allowed, n_affected, replace=False)).astype(np.int32)
    owner = rng.randint(0, n_targets, n_affected)                 # the one target that names the corner for sure
    targets = []
    for t in range(n_targets):
        # a few corners per target beyond its own: with 1024 targets the table stays small
        p = min(1.0, max(0.35 if n_targets <= 8 else 0.0, 3.0 / max(n_affected, 1)))
        named = (owner == t) | (rng.uniform(size=n_affected) < p)
        if all_targets_corner and n_affected:
            named[0] = True
        c = affected[named]
        rng.shuffle(c)
        targets.append((c.astype(np.int32), rng.uniform(-scale, scale, (c.size, 6)).astype(f32)))
    return targets, affected


def special_weights(n_targets, seed=4):
    """+0, -0, denormals, negatives, 2.0 and ordinary weights"""
    rng = np.random.RandomState(seed)
    special = np.array([0.0, -0.0, 1e-45, -1e-39, -0.75, 2.0, 1.0], f32)
    w = rng.uniform(-1.0, 1.5, n_targets).astype(f32)
    pick = rng.randint(0, 2 * special.size, n_targets)
    w = np.where(pick < special.size, special[np.minimum(pick, special.size - 1)], w).astype(f32)
    if n_targets >= special.size:
        w[:special.size] = special
    return w


def flat(targets):
    """the C arrays of pt_morph_attach: (target_start int64, entry_corner int32, entry_delta float32)"""
    start = np.zeros(len(targets) + 1, np.int64)
    start[1:] = np.cumsum([len(c) for c, _ in targets])
    corner = np.concatenate([np.asarray(c, np.int32).reshape(-1) for c, _ in targets] + [np.zeros(0, np.int32)])
    delta = np.concatenate([np.asarray(d, f32).reshape(-1) for _, d in targets] + [np.zeros(0, f32)])
    return start, corner, delta


def rows(targets, n_corners):
    """ptp::morphRows, stated a second time: (affected corners ascending, row starts, per entry its target, per entry its six floats)"""
    start, corner, delta = flat(targets)
    target = np.repeat(np.arange(len(targets)), np.diff(start))
    order = np.lexsort((target, corner))
    affected, count = np.unique(corner, return_counts=True)
    assert affected.size == 0 or affected.max() < n_corners
    return affected.astype(np.int32), np.concatenate([[0], np.cumsum(count)]).astype(np.int32), target[order].astype(np.int32), delta.reshape(-1, 6)[order]


def shared_corners_crack(tris, rest, targets, words):
    """the number of corner pairs with equal rest floats, equal entries (target, delta) and equal skin or part words (`words`: one bytes object per
    corner) whose posed floats differ in a bit -> (cracks, shared pairs that carry entries)"""
    rest = np.ascontiguousarray(rest, f32).reshape(-1, 40).view(np.uint32)
    out = np.ascontiguousarray(tris, f32).reshape(-1, 40).view(np.uint32)
    entries = {}
    for t, (corners, deltas) in enumerate(targets):
        d = np.ascontiguousarray(deltas, f32).reshape(-1, 6)
        for q, row in zip(np.asarray(corners).reshape(-1), d):
            entries.setdefault(int(q), []).append((t, row.tobytes()))
    seen, cracks, shared = {}, 0, 0
    for k in range(rest.shape[0]):
        for c in range(3):
            q = 3 * k + c
            key = (rest[k, 4 * c:4 * c + 3].tobytes(), rest[k, 12 + 4 * c:15 + 4 * c].tobytes(), tuple(entries.get(q, ())), words[q])
            got = (out[k, 4 * c:4 * c + 3].tobytes(), out[k, 12 + 4 * c:15 + 4 * c].tobytes())
            if key in seen:
                shared += q in entries
                cracks += seen[key] != got
            else:
                seen[key] = got
    return cracks, shared
