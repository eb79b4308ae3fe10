"""The rule of include/pt_normals.h in numpy binary32: the face vector of every listed triangle (every product rounded before every difference),
per vertex the sequential sum over its corners in ascending corner index, the correctly rounded length and divide, the fallback; composed with
the pose, skin and morph models (the normals step runs last).  Also the two evaluations the rule is NOT (fused, and binary64 rounded once), so that
a test can show the comparison tells them apart, and the cases the CPU and GPU tests share."""
import numpy as np

import _morph_model as MM
import _pose_model as PM
import _skin_model as SM

f32 = np.float32


def rows(corner_vertex, n_vertices=None):
    """ptp::normalRows, stated a second time: (listed triangles ascending, non-empty ids ascending, row starts, corners by (id, corner), per
    corner its row)"""
    ids = np.asarray(corner_vertex, np.int64).reshape(-1)
    q = np.nonzero(ids >= 0)[0]
    order = q[np.argsort(ids[q], kind="stable")]                  # ascending id, within an id ascending corner
    verts, count = np.unique(ids[q], return_counts=True)
    assert n_vertices is None or verts.size == 0 or verts.max() < n_vertices
    start = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    return (np.unique(q // 3).astype(np.int32), verts.astype(np.int32), start, order.astype(np.int32),
            np.repeat(np.arange(verts.size), count).astype(np.int32))


def faces(tris, flip=False):
    """the face vector of every triangle: (n, 3) float32"""
    t = np.ascontiguousarray(tris, f32).reshape(-1, 40)
    with np.errstate(all="ignore"):
        e1 = (t[:, 4:7] - t[:, 0:3]).astype(f32)
        e2 = (t[:, 8:11] - t[:, 0:3]).astype(f32)
        F = np.empty((t.shape[0], 3), f32)
        for j, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
            F[:, j] = ((e1[:, a] * e2[:, b]).astype(f32) - (e1[:, b] * e2[:, a]).astype(f32)).astype(f32)
    return -F if flip else F


def smooth(tris, corner_vertex, flip=False, faces_of=faces, want_fallbacks=False):
    """tris: 40 floats per triangle as the pose's rule wrote them -> the same with the normals of the corners with an id >= 0 recomputed.
    want_fallbacks: -> (that, the ids that took the fallback)"""
    out = np.ascontiguousarray(tris, f32).reshape(-1, 40).copy()
    _, verts, start, order, _ = rows(corner_vertex)
    fell = np.zeros(0, np.int32)
    if verts.size:
        F = faces_of(out, flip)
        count = np.diff(start)
        with np.errstate(all="ignore"):
            S = F[order[start[:-1]] // 3].copy()                  # S = F[q_0 / 3]
            for r in range(1, int(count.max())):                  # then the r-th corner of every row that has one, r ascending: a sequential sum per row
                has = np.nonzero(count > r)[0]
                S[has] = (S[has] + F[order[start[has] + r] // 3]).astype(f32)
            sq = (S * S).astype(f32)
            L = np.sqrt(((sq[:, 0] + sq[:, 1]).astype(f32) + sq[:, 2]).astype(f32)).astype(f32)
            ok = np.isfinite(L) & (L > 0)
            N = (S / np.where(ok, L, f32(1.0))[:, None]).astype(f32)
        fell = verts[~ok]
        row_of = np.repeat(np.arange(verts.size), count)
        keep = ok[row_of]
        q = order[keep].astype(np.int64)
        k, c = q // 3, q % 3
        for j in range(3):
            out[k, 12 + 4 * c + j] = N[row_of[keep], j]
    return (out.reshape(-1), fell) if want_fallbacks else out.reshape(-1)


def faces_f64(tris, flip=False):
    """what the rule is not: the cross product in binary64, rounded once"""
    t = np.ascontiguousarray(tris, f32).reshape(-1, 40).astype(np.float64)
    F = np.cross(t[:, 4:7] - t[:, 0:3], t[:, 8:11] - t[:, 0:3]).astype(f32)
    return -F if flip else F


def faces_fma(tris, flip=False):
    """what the rule is not: a * b - c * d as fma(a, b, -(c * d)), the chain a compiler contracts it to"""
    t = np.ascontiguousarray(tris, f32).reshape(-1, 40)
    e1 = (t[:, 4:7] - t[:, 0:3]).astype(f32)
    e2 = (t[:, 8:11] - t[:, 0:3]).astype(f32)
    F = np.empty((t.shape[0], 3), f32)
    for k in range(t.shape[0]):
        for j, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
            F[k, j] = PM._fma(e1[k, a], e2[k, b], -f32(e1[k, b] * e2[k, a]))
    return -F if flip else F


def pose_smooth(rest, tri_part, xforms, corner_vertex, flip=False):
    """pt_pose_triangles of a pose of pt_pose_create with normals"""
    return smooth(PM.pose(rest, tri_part, xforms), corner_vertex, flip)


def skin_smooth(rest, bone, weight, xforms, corner_vertex, flip=False):
    """pt_pose_triangles of a pose of pt_skin_create with normals"""
    return smooth(SM.skin(rest, bone, weight, xforms), corner_vertex, flip)


def morph_skin_smooth(rest, targets, weights, bone, weight, xforms, corner_vertex, flip=False):
    """the whole chain: morph -> skin -> normals"""
    return smooth(MM.morph_skin(rest, targets, weights, bone, weight, xforms), corner_vertex, flip)


def random_ids(allowed, n_vertices, seed=3, minus=0.2, n_tris=None):
    """ids for the corners `allowed` (3 * k + c, ascending): each draws one of n_vertices ids, or -1 with probability `minus`; within a triangle
    an id stands once (a repeat becomes -1).  Every other corner gets -1.  -> corner_vertex int32[3 * n_tris]"""
    rng = np.random.RandomState(seed)
    allowed = np.asarray(allowed, np.int64)
    n_tris = (int(allowed.max()) // 3 + 1 if allowed.size else 0) if n_tris is None else n_tris
    ids = np.full(3 * n_tris, -1, np.int32)
    if n_vertices:
        g = rng.randint(0, n_vertices, allowed.size).astype(np.int32)
        g[rng.uniform(size=allowed.size) < minus] = -1
        ids[allowed] = g
    t = ids.reshape(-1, 3)
    t[(t[:, 1] == t[:, 0]), 1] = -1
    t[(t[:, 2] == t[:, 0]) | (t[:, 2] == t[:, 1]), 2] = -1
    return ids


def ids_counted(n_tris, m):
    """ids with exactly m listed triangles (the first m) and m non-empty vertices, rows of uneven length: corner 0 of triangle k names vertex k,
    corner 1 vertex k + 1 (mod m), corner 2 a scattered one where that is a third vertex, else -1.  Every corner of the first m triangles must be
    one the pose's rule moves."""
    ids = np.full(3 * n_tris, -1, np.int32)
    k = np.arange(m)
    ids[3 * k] = k
    if m > 1:
        ids[3 * k + 1] = (k + 1) % m
        third = (k * 7 + 3) % m
        ids[3 * k + 2] = np.where((third != k) & (third != (k + 1) % m) & (k % 3 != 0), third, -1)
    return ids


def angle_deg(a, b):
    """per row the angle between two vectors, degrees, in binary64"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    c = (a * b).sum(axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))


def sine_grid(n=32, amp=0.08):
    """The quality statement's surface: an n x n-cell grid over the unit square, each cell split along (i, j)-(i + 1, j + 1), vertices at
    z = amp sin(2 pi x) sin(2 pi y), the rest normals (0, 0, 1) carried through (a morph without normal deltas under an identity pose).
    -> (tris 40 floats per triangle, corner_vertex, per corner the analytic normal (3 n_tris, 3))"""
    idx = lambda i, j: i * (n + 1) + j
    cells = [(i, j) for i in range(n) for j in range(n)]
    vid = np.array([[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)] for i, j in cells] + [[idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)] for i, j in cells], np.int32)
    gi, gj = np.divmod(np.arange((n + 1) ** 2), n + 1)
    x, y = gi / n, gj / n
    z = amp * np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y)
    pos = np.stack([x, y, z], axis=1).astype(f32)
    dzdx = amp * 2 * np.pi * np.cos(2 * np.pi * x) * np.sin(2 * np.pi * y)
    dzdy = amp * 2 * np.pi * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y)
    exact = np.stack([-dzdx, -dzdy, np.ones_like(x)], axis=1)
    exact /= np.linalg.norm(exact, axis=1)[:, None]
    t = np.zeros((vid.shape[0], 40), f32)
    for c in range(3):
        t[:, 4 * c:4 * c + 3] = pos[vid[:, c]]
        t[:, 12 + 4 * c:12 + 4 * c + 3] = (0.0, 0.0, 1.0)
    return t.reshape(-1), vid.reshape(-1), exact[vid.reshape(-1)]


def corner_normals(tris):
    t = np.ascontiguousarray(tris, f32).reshape(-1, 40)
    return np.stack([t[:, 12 + 4 * c:12 + 4 * c + 3] for c in range(3)], axis=1).reshape(-1, 3)
