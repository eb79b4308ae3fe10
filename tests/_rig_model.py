"""include/pt_rig.h's rule in numpy binary32, written from the header and not from the C++: every array is float32 and every numpy operation
rounds once, so a * b + c below is a rounded product and a rounded sum, in the order written.  Also the helpers the rig tests share: the
hierarchies and locals of the listed cases."""
import numpy as np

f32 = np.float32
MAX_DEPTH = 256


def depths(parent):
    parent = np.asarray(parent, np.int64)
    d = np.zeros(parent.size, np.int64)
    for j, p in enumerate(parent):
        d[j] = 1 if p < 0 else d[p] + 1
    return d


def level_plan(parent):
    """(order, level_start): the joints by (depth, id); level l holds the joints of depth l + 1"""
    d = depths(parent)
    order = np.lexsort((np.arange(d.size), d)).astype(np.int32)
    levels = int(d.max()) if d.size else 0
    start = np.concatenate([[0], np.cumsum(np.bincount(d, minlength=levels + 1)[1:])]).astype(np.int32)
    return order, start


def local_matrices(locals_):
    """step 1: (n, 3, 4) float32"""
    l = np.ascontiguousarray(locals_, f32).reshape(-1, 12)
    one, two = f32(1.0), f32(2.0)
    with np.errstate(all="ignore"):
        x, y, z, w = l[:, 4], l[:, 5], l[:, 6], l[:, 7]
        n = np.sqrt(((x * x + y * y) + z * z) + w * w)
        x, y, z, w = x / n, y / n, z / n, w / n
        xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        R = np.stack([one - two * (yy + zz), two * (xy - wz), two * (xz + wy),
                      two * (xy + wz), one - two * (xx + zz), two * (yz - wx),
                      two * (xz - wy), two * (yz + wx), one - two * (xx + yy)], axis=1).reshape(-1, 3, 3)
        L = np.zeros((l.shape[0], 3, 4), f32)
        L[:, :, :3] = R * l[:, None, 8:11]
        L[:, :, 3] = l[:, 0:3]
    return L


def compose(A, B):
    """A o B on (n, 3, 4) float32 arrays"""
    C = np.zeros_like(A)
    with np.errstate(all="ignore"):
        for i in range(3):
            for k in range(4):
                s = (A[:, i, 0] * B[:, 0, k] + A[:, i, 1] * B[:, 1, k]) + A[:, i, 2] * B[:, 2, k]
                C[:, i, k] = s if k < 3 else s + A[:, i, 3]
    return C


def records_of(M):
    """step 4: (n, 24) float32 from (n, 3, 4)"""
    out = np.zeros((M.shape[0], 24), f32)
    out[:, :12] = M.reshape(-1, 12)
    c = np.zeros((M.shape[0], 3, 3), f32)
    with np.errstate(all="ignore"):
        for i in range(3):
            for k in range(3):
                i1, i2, k1, k2 = (i + 1) % 3, (i + 2) % 3, (k + 1) % 3, (k + 2) % 3
                c[:, i, k] = M[:, i1, k1] * M[:, i2, k2] - M[:, i1, k2] * M[:, i2, k1]
        det = (M[:, 0, 0] * c[:, 0, 0] + M[:, 0, 1] * c[:, 0, 1]) + M[:, 0, 2] * c[:, 0, 2]
        out[:, 12:21] = (c / det[:, None, None]).reshape(-1, 9)
    return out


def world(parent, locals_):
    """steps 1 and 2: (n, 3, 4) float32, level by level"""
    parent = np.asarray(parent, np.int64)
    L = local_matrices(locals_)
    W = np.zeros_like(L)
    order, start = level_plan(parent)
    for l in range(len(start) - 1):
        js = order[start[l]:start[l + 1]].astype(np.int64)
        W[js] = L[js] if l == 0 else compose(W[parent[js]], L[js])
    return W


def records(parent, locals_, inv_bind=None):
    """steps 1-4: (n, 24) float32"""
    W = world(parent, locals_)
    if inv_bind is not None and W.shape[0]:
        W = compose(W, np.ascontiguousarray(inv_bind, f32).reshape(-1, 3, 4))
    return records_of(W)


def interval(times, t):
    """step 5, the host's part: (exact key or -1, k, u)"""
    T = np.ascontiguousarray(times, f32)
    t = f32(t)
    if T.size == 1:
        return 0, 0, f32(0)
    t = min(max(t, T[0]), T[-1])
    k = 0
    while k < T.size - 2 and t >= T[k + 1]:
        k += 1
    u = f32(f32(t - T[k]) / f32(T[k + 1] - T[k]))
    if u == 0:
        return k, k, u
    if u == 1:
        return k + 1, k, u
    return -1, k, u


def blend(a, b, u):
    """step 5, the blend of two keys' locals (n, 12) under u"""
    a, b = np.ascontiguousarray(a, f32).reshape(-1, 12), np.ascontiguousarray(b, f32).reshape(-1, 12)
    u = f32(u)
    v = f32(1.0) - u
    with np.errstate(all="ignore"):
        d = ((a[:, 4] * b[:, 4] + a[:, 5] * b[:, 5]) + a[:, 6] * b[:, 6]) + a[:, 7] * b[:, 7]
        uq = np.where(d < 0, -u, u).astype(f32)
        out = v * a + u * b
        out[:, 4:8] = v * a[:, 4:8] + uq[:, None] * b[:, 4:8]
    return out


def flips(a, b):
    """per joint: the blend of these two keys negates b's quaternion"""
    a, b = np.ascontiguousarray(a, f32).reshape(-1, 12), np.ascontiguousarray(b, f32).reshape(-1, 12)
    return (((a[:, 4] * b[:, 4] + a[:, 5] * b[:, 5]) + a[:, 6] * b[:, 6]) + a[:, 7] * b[:, 7]) < 0


def clip_locals(times, values, n, t):
    V = np.ascontiguousarray(values, f32).reshape(len(times), n, 12)
    exact, k, u = interval(times, t)
    return V[exact] if exact >= 0 else blend(V[k], V[k + 1], u)


def clip_records(parent, times, values, t, inv_bind=None):
    n = np.asarray(parent).size
    return records(parent, clip_locals(times, values, n, t), inv_bind)


# ------------------------------------------------------------------------------------------------ the cases

def random_locals(n, seed, scale=(0.5, 1.5), shift=1.0, unnormalised=True):
    """t in [-shift, shift], q a random direction (times a length in [0.3, 3] when unnormalised), s in `scale` with random signs kept positive;
    the paddings hold NaN: they are never read"""
    rng = np.random.RandomState(seed)
    l = np.zeros((n, 12), f32)
    l[:, 0:3] = rng.uniform(-shift, shift, (n, 3))
    q = rng.normal(0, 1, (n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    if unnormalised:
        q *= rng.uniform(0.3, 3.0, (n, 1))
    l[:, 4:8] = q
    l[:, 8:11] = rng.uniform(scale[0], scale[1], (n, 3))
    l[:, 3] = l[:, 11] = np.nan
    return l


def random_binds(n, seed):
    """inverse bind matrices: rotations with shifts, rounded once"""
    l = random_locals(n, seed + 1000, scale=(1.0, 1.0), unnormalised=False)
    return local_matrices(l).reshape(n, 12)


def chain(n):
    return np.arange(-1, n - 1, dtype=np.int32)


def star(n_children):
    return np.concatenate([[-1], np.zeros(n_children, np.int32)]).astype(np.int32)


def forest(n, seed, roots_at_end=3, max_depth=MAX_DEPTH):
    """random parents in [-1, j), about one joint in 40 a root, and the last roots_at_end joints roots too"""
    rng = np.random.RandomState(seed)
    parent = np.full(n, -1, np.int32)
    for j in range(1, n - roots_at_end):
        if rng.uniform() > 0.025:
            parent[j] = rng.randint(max(0, j - 30), j)
    assert depths(parent).max() <= max_depth
    return parent


def hierarchies():
    """(tag, parent) of the cases the issue lists, n_parts == 0 included"""
    return [("one", chain(1)), ("two", chain(2)), ("chain65", chain(65)), ("star300", star(300)), ("forest1000", forest(1000, 7)),
            ("depth256", chain(MAX_DEPTH)), ("none", np.zeros(0, np.int32))]


def case_locals(tag, n, seed=0):
    """the locals of a case: unnormalised q throughout; a chain keeps its scale near 1 so that 256 levels stay finite.  `zero` adds a zero scale"""
    deep = tag.startswith("depth") or tag.startswith("chain")
    wide = tag.startswith("forest")                                   # (some sixty levels: scales that keep the products well conditioned)
    return random_locals(n, seed + n, scale=(0.98, 1.02) if deep else (0.8, 1.25) if wide else (0.5, 1.5), shift=0.1 if deep else 1.0)


def with_zero_scale(l):
    l = l.copy()
    l[l.shape[0] // 2, 8] = 0.0                                       # one joint's s.x: its subtree's M is singular
    return l


def same_floats(got, want):
    """bit for bit, but a NaN the rule generates equals any NaN: its sign and payload are the hardware's"""
    g, w = np.ascontiguousarray(got, f32).reshape(-1), np.ascontiguousarray(want, f32).reshape(-1)
    assert g.shape == w.shape, (g.shape, w.shape)
    same = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
    return bool(same.all()), int((~same).sum())
