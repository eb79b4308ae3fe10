"""The rule of include/pt_pose.h in numpy binary32: every product rounded before every sum, in the header's written order.  Also the two
evaluations the rule is NOT (a fused multiply-add chain, binary64 then rounded), so that a test can show it tells them apart, and the cases the
CPU and GPU tests share."""
import numpy as np

f32 = np.float32
REC = 24


def pose(rest, tri_part, xforms):
    """rest: 40 floats per triangle; tri_part: int per triangle in [-1, n_parts); xforms: n_parts records of 24 floats -> the posed binding 3"""
    rest = np.ascontiguousarray(rest, f32).reshape(-1, 40)
    part = np.asarray(tri_part, np.int64).reshape(-1)
    assert part.size == rest.shape[0]
    out = rest.copy()
    X = np.ascontiguousarray(xforms, f32).reshape(-1, REC)
    moving = np.nonzero(part >= 0)[0]
    if moving.size == 0:
        return out.reshape(-1)
    R = X[part[moving]]                                  # one record per moving triangle
    M = R[:, :12].reshape(-1, 3, 4)
    N = R[:, 12:21].reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        for q in range(6):
            v = rest[moving, 4 * q:4 * q + 3]
            A = M if q < 3 else N
            for i in range(3):
                a = (A[:, i, 0] * v[:, 0]).astype(f32)
                b = (A[:, i, 1] * v[:, 1]).astype(f32)
                c = (A[:, i, 2] * v[:, 2]).astype(f32)
                s = ((a + b).astype(f32) + c).astype(f32)
                if q < 3:
                    s = (s + M[:, i, 3]).astype(f32)
                out[moving, 4 * q + i] = s
    return out.reshape(-1)


def pose_f64(rest, tri_part, xforms):
    """what the rule is not: every sum in binary64, rounded once"""
    rest = np.ascontiguousarray(rest, f32).reshape(-1, 40)
    part = np.asarray(tri_part, np.int64).reshape(-1)
    out = rest.copy()
    X = np.ascontiguousarray(xforms, f32).reshape(-1, REC).astype(np.float64)
    for k in np.nonzero(part >= 0)[0]:
        M = X[part[k], :12].reshape(3, 4); N = X[part[k], 12:21].reshape(3, 3)
        for q in range(6):
            v = rest[k, 4 * q:4 * q + 3].astype(np.float64)
            out[k, 4 * q:4 * q + 3] = (M[:, :3] @ v + M[:, 3]) if q < 3 else (N @ v)
    return out.reshape(-1)


def _fma(a, b, c):
    """round(a * b + c) of binary32 inputs: the product of two binary32 is exact in binary64, and the binary64 sum's double rounding cannot show
    for the inputs used here (checked where it is used against exact rational arithmetic)"""
    from fractions import Fraction
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    lo = f32(float(exact))                               # float(Fraction) rounds correctly to binary64; then to binary32: guard the double rounding
    cands = [lo, np.nextafter(lo, f32(-np.inf)), np.nextafter(lo, f32(np.inf))]
    return min(cands, key=lambda x: (abs(Fraction(float(x)) - exact), int(x.view(np.uint32)) & 1))


def pose_fma(rest, tri_part, xforms):
    """what the rule is not: the chain a compiler contracts it to, fma(m2, z, fma(m1, y, m0 * x)) + m3 with the last sum fused as well"""
    rest = np.ascontiguousarray(rest, f32).reshape(-1, 40)
    part = np.asarray(tri_part, np.int64).reshape(-1)
    out = rest.copy()
    X = np.ascontiguousarray(xforms, f32).reshape(-1, REC)
    for k in np.nonzero(part >= 0)[0]:
        M = X[part[k], :12].reshape(3, 4); N = X[part[k], 12:21].reshape(3, 3)
        for q in range(6):
            v = rest[k, 4 * q:4 * q + 3]
            for i in range(3):
                A = M[i] if q < 3 else N[i]
                s = _fma(A[2], v[2], _fma(A[1], v[1], f32(A[0] * v[0])))
                out[k, 4 * q + i] = f32(s + M[i][3]) if q < 3 else s
    return out.reshape(-1)


def rotation(axis, angle, shift=(0.0, 0.0, 0.0), scale=1.0):
    """a 3 x 4 matrix in binary64: rotation about `axis` by `angle`, uniform scale, then the shift"""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    return np.concatenate([scale * R, np.asarray(shift, np.float64).reshape(3, 1)], axis=1)


def records(M, N=None):
    """renderer.pose_records, stated a second time"""
    M = np.asarray(M, np.float64).reshape(-1, 3, 4)
    if N is None:
        N = np.array([np.linalg.inv(m[:, :3]).T for m in M]).reshape(-1, 3, 3)
    out = np.zeros((len(M), REC), f32)
    out[:, :12] = M.reshape(len(M), 12)
    out[:, 12:21] = np.asarray(N, np.float64).reshape(len(M), 9)
    return out


def matrices(n_parts, seed=5):
    """n_parts rotations with shifts and scales: records of 24 floats (padding set to a NaN, which the rule ignores)"""
    rng = np.random.RandomState(seed)
    M = [rotation(rng.normal(size=3), rng.uniform(-0.6, 0.6), rng.uniform(-0.3, 0.3, 3), rng.uniform(0.8, 1.25)) for _ in range(n_parts)]
    X = records(np.array(M).reshape(-1, 3, 4))
    X[:, 21:] = np.nan
    return X


def parts_mod4(n_tris):
    """the tests' assignment: k % 4 - 1, so a quarter is static and three parts move"""
    return (np.arange(n_tris) % 4 - 1).astype(np.int32)


SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, np.inf, -np.inf, 3e38, -3e38, 1.0, -2.5], f32)


def special_triangles(n, seed=3):
    """n triangles whose vertex and normal floats are drawn from SPECIAL and ordinary values (floats 24-39 ordinary, material index 0)"""
    rng = np.random.RandomState(seed)
    t = rng.uniform(-2, 2, (n, 40)).astype(f32)
    pick = rng.randint(0, SPECIAL.size + 6, (n, 24))
    with np.errstate(all="ignore"):
        t[:, :24] = np.where(pick < SPECIAL.size, SPECIAL[np.minimum(pick, SPECIAL.size - 1)], t[:, :24])
    t[:, 36] = 0.0
    return t.reshape(-1)
