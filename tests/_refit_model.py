"""numpy model of include/pt_refit.h: float32 boxes in the order in which -0.0 < +0.0, float64 cost in the written order, bottom-up.  It does what the
header says and nothing else: no refusals but an assertion where the walk would leave the buffers (csrc/hip/pt_refit_plan.hpp owns the refusals)."""
import numpy as np

f32 = np.float32


def key(x):
    """order-preserving uint32 keys of float32 values: -0.0 < +0.0, as Java's Math.min / Math.max order them (no NaN among the inputs)"""
    b = np.ascontiguousarray(x, dtype=f32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k >> 31 != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(f32)


def vertices(tris):
    """binding 3 -> (n, 3 vertices, 3) float32: floats 0-2, 4-6 and 8-10 of each 40-float record"""
    t = np.ascontiguousarray(tris, dtype=f32).reshape(-1, 40)
    return np.stack([t[:, 0:3], t[:, 4:7], t[:, 8:11]], axis=1)


def area(mn, mx):
    s = mx.astype(np.float64) - mn.astype(np.float64)
    return (s[0] * s[1] + s[0] * s[2]) + s[1] * s[2]


def structure(data, tree, roots):
    """(parent, height, reachable ids in an order in which children come first) of the nodes the roots reach; height -1 elsewhere"""
    tree = np.asarray(tree, np.int32).reshape(-1, 3)
    n = len(tree)
    parent, height = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    roots = np.asarray(roots, np.int32)
    todo, post = [int(r) for r in roots[1:1 + int(roots[0])]], []
    seen = set()
    while todo:
        i = todo.pop()
        assert 0 <= i < n and i not in seen
        seen.add(i)
        post.append(i)
        left, right = int(tree[i, 1]), int(tree[i, 2])
        if left == -1 and right == -1:
            continue
        parent[left] = parent[right] = i
        todo += [left, right]
    for i in reversed(post):                         # a node is appended before its children: reversed, children come first
        left, right = int(tree[i, 1]), int(tree[i, 2])
        height[i] = 0 if left == -1 and right == -1 else 1 + max(height[left], height[right])
    return parent, height, post[::-1]


def refit(data, tree, leaf_tris, roots, tris, want_nan_check=True):
    """-> (binding 10 after the refit, root_cost), or None when a referenced triangle holds a NaN"""
    data = np.ascontiguousarray(data, dtype=f32).reshape(-1, 8)
    tree = np.asarray(tree, np.int32).reshape(-1, 3)
    leaf_tris = np.asarray(leaf_tris, np.int32)
    roots = np.asarray(roots, np.int32)
    v = vertices(tris)
    kv = key(v)
    out = data.copy()
    S = np.zeros(len(tree), np.float64)
    _, _, order = structure(data, tree, roots)
    with np.errstate(all="ignore"):
        for i in order:
            left, right = int(tree[i, 1]), int(tree[i, 2])
            if left == -1 and right == -1:
                s, e = int(data[i, 6]), int(data[i, 7])
                assert s == data[i, 6] and e == data[i, 7] and 0 <= s <= e <= len(leaf_tris)
                if e > s:
                    ids = leaf_tris[s:e]
                    assert (ids >= 0).all() and (ids < len(v)).all()
                    if want_nan_check and np.isnan(v[ids]).any():
                        return None
                    k = kv[ids].reshape(-1, 3)
                    out[i, 0:3], out[i, 3:6] = unkey(k.min(axis=0)), unkey(k.max(axis=0))
                S[i] = area(out[i, 0:3], out[i, 3:6]) * np.float64(e - s)
            else:
                out[i, 0:3] = unkey(np.minimum(key(out[left, 0:3]), key(out[right, 0:3])))
                out[i, 3:6] = unkey(np.maximum(key(out[left, 3:6]), key(out[right, 3:6])))
                S[i] = area(out[i, 0:3], out[i, 3:6]) + (S[left] + S[right])
    cost = np.array([S[int(r)] for r in roots[1:1 + int(roots[0])]], np.float64)
    return out.reshape(-1), cost


def refit_buffers(b, tris=None):
    """the model on a workload's buffers {10, 11, 12, 13}, with its own binding 3 unless another is given"""
    return refit(b[10], b[11], b[12], b[13], b[3] if tris is None else tris)
