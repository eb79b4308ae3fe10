"""The rule of include/pt_skin_dq.h in numpy binary32, every intermediate rounded: per record its dual quaternion (step 1), per corner the blend
about slot 0's real part, normalised (step 2), the record B the blend turns back into (step 3), then tests/_pose_model.py's arithmetic (PM.pose
with one "part" per corner) on B (step 4).  numpy's binary32 product, sum, quotient and square root are the correctly rounded ones, and no
expression here is fused.  Also the two evaluations the rule is NOT (fused, and binary64 rounded once), and the cases the CPU and GPU tests share."""
import numpy as np

import _pose_model as PM

f32 = np.float32
REC = PM.REC
ONE, TWO, HALF, QUARTER = f32(1.0), f32(2.0), f32(0.5), f32(0.25)


def dq_from_records(xforms):
    """records of 24 floats -> (Q (n, 8) binary32, branch (n,) in 0..3: the trace, then the largest diagonal m00 / m11 / m22)"""
    X = np.ascontiguousarray(xforms, f32).reshape(-1, REC)
    m00, m01, m02, tx, m10, m11, m12, ty, m20, m21, m22, tz = (X[:, j] for j in range(12))
    with np.errstate(all="ignore"):
        tr = (m00 + m11) + m22
        branch = np.where(tr > 0, 0, np.where((m00 > m11) & (m00 > m22), 1, np.where(m11 > m22, 2, 3)))
        s = [np.sqrt(tr + ONE) * TWO, np.sqrt(((ONE + m00) - m11) - m22) * TWO, np.sqrt(((ONE + m11) - m00) - m22) * TWO, np.sqrt(((ONE + m22) - m00) - m11) * TWO]
        w = [QUARTER * s[0], (m21 - m12) / s[1], (m02 - m20) / s[2], (m10 - m01) / s[3]]
        x = [(m21 - m12) / s[0], QUARTER * s[1], (m01 + m10) / s[2], (m02 + m20) / s[3]]
        y = [(m02 - m20) / s[0], (m01 + m10) / s[1], QUARTER * s[2], (m12 + m21) / s[3]]
        z = [(m10 - m01) / s[0], (m02 + m20) / s[1], (m12 + m21) / s[2], QUARTER * s[3]]
        w, x, y, z = (np.choose(branch, v).astype(f32) for v in (w, x, y, z))
        n = np.sqrt(((w * w + x * x) + y * y) + z * z)
        w, x, y, z = w / n, x / n, y / n, z / n
        Q = np.zeros((X.shape[0], 8), f32)
        Q[:, 0], Q[:, 1], Q[:, 2], Q[:, 3] = w, x, y, z
        Q[:, 4] = -HALF * ((tx * x + ty * y) + tz * z)
        Q[:, 5] = HALF * ((tx * w + ty * z) - tz * y)
        Q[:, 6] = HALF * ((ty * w + tz * x) - tx * z)
        Q[:, 7] = HALF * ((tz * w + tx * y) - ty * x)
    assert Q.dtype == f32
    return Q, branch


def blend(bone, weight, Q):
    """bone, weight: (n_corners, 4); Q: the table -> (r, d, flips): the normalised blend (n_corners, 4) each (rows of static corners: NaN) and
    per slot whether its weight was negated"""
    bone = np.asarray(bone, np.int64).reshape(-1, 4)
    w = np.ascontiguousarray(weight, f32).reshape(-1, 4)
    n = bone.shape[0]
    Br, Bd = np.zeros((n, 4), f32), np.zeros((n, 4), f32)
    flips = np.zeros((n, 4), bool)
    use = bone[:, 0] >= 0
    with np.errstate(all="ignore"):
        if use.any():
            q0 = np.zeros((n, 8), f32)
            q0[use] = Q[bone[use, 0]]
            Br[use] = w[use, 0, None] * q0[use, :4]
            Bd[use] = w[use, 0, None] * q0[use, 4:]
            for s in (1, 2, 3):
                use = use & (bone[:, s] >= 0)                  # the slots are packed: the first empty one ends the corner
                at = np.nonzero(use)[0]
                if at.size == 0:
                    break
                qs = Q[bone[at, s]]
                p = q0[at, :4] * qs[:, :4]
                dot = ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]
                flips[at, s] = dot < 0
                ws = np.where(dot < 0, -w[at, s], w[at, s]).astype(f32)
                Br[at] = Br[at] + ws[:, None] * qs[:, :4]
                Bd[at] = Bd[at] + ws[:, None] * qs[:, 4:]
        L = np.sqrt(((Br[:, 0] * Br[:, 0] + Br[:, 1] * Br[:, 1]) + Br[:, 2] * Br[:, 2]) + Br[:, 3] * Br[:, 3])
        r, d = Br / L[:, None], Bd / L[:, None]
    assert r.dtype == f32 and d.dtype == f32
    return r, d, flips


def dq_record(r, d):
    """the normalised blends -> (n, 24) records B: M = [R | t], N = R, padding 0"""
    w, x, y, z = (r[:, j] for j in range(4))
    dw, dx, dy, dz = (d[:, j] for j in range(4))
    B = np.zeros((r.shape[0], REC), f32)
    with np.errstate(all="ignore"):
        xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
        R = [ONE - TWO * (yy + zz), TWO * (xy - wz), TWO * (xz + wy),
             TWO * (xy + wz), ONE - TWO * (xx + zz), TWO * (yz - wx),
             TWO * (xz - wy), TWO * (yz + wx), ONE - TWO * (xx + yy)]
        t = [TWO * (((dx * w - dw * x) + dz * y) - dy * z), TWO * (((dy * w - dw * y) + dx * z) - dz * x), TWO * (((dz * w - dw * z) + dy * x) - dx * y)]
    for i in range(3):
        for j in range(3):
            B[:, 4 * i + j] = R[3 * i + j]
            B[:, 12 + 3 * i + j] = R[3 * i + j]
        B[:, 4 * i + 3] = t[i]
    return B


def corner_records(bone, weight, xforms, info=None):
    """steps 1-3: one record B per corner (n_corners, 24).  info (a dict) receives branch (per record), flips (per corner and slot), Q, r, d"""
    Q, branch = dq_from_records(xforms)
    r, d, flips = blend(bone, weight, Q)
    if info is not None:
        info.update(branch=branch, flips=flips, Q=Q, r=r, d=d)
    return dq_record(r, d)


def pose_corners(rest, bone, B):
    """step 4: rest (40 floats per triangle) under one record per corner, static corners kept; PM.pose's arithmetic"""
    rest = np.ascontiguousarray(rest, f32).reshape(-1, 40)
    n = rest.shape[0]
    out = rest.copy()
    part = np.where(np.asarray(bone, np.int64).reshape(n, 3, 4)[:, :, 0].reshape(-1) >= 0, np.arange(3 * n), -1)
    for c in range(3):
        posed = PM.pose(rest, part.reshape(n, 3)[:, c], B).reshape(n, 40)      # "triangle" k under "part" 3k + c: only corner c's two float4 are kept
        out[:, 4 * c:4 * c + 3] = posed[:, 4 * c:4 * c + 3]
        out[:, 12 + 4 * c:12 + 4 * c + 3] = posed[:, 12 + 4 * c:12 + 4 * c + 3]
    return out.reshape(-1)


def skin_dq(rest, bone, weight, xforms, info=None):
    """rest: 40 floats per triangle; bone, weight: 12 per triangle; xforms: records of 24 floats -> the posed binding 3"""
    rest = np.ascontiguousarray(rest, f32).reshape(-1, 40)
    if rest.shape[0] == 0:
        return rest.reshape(-1).copy()
    bone = np.asarray(bone, np.int64).reshape(-1, 4)
    if np.ascontiguousarray(xforms, f32).size == 0:
        assert (bone < 0).all()
        return rest.reshape(-1).copy()
    B = corner_records(bone, np.ascontiguousarray(weight, f32).reshape(-1, 4), xforms, info)
    return pose_corners(rest, bone, B)


# ---- what the rule is not

def skin_dq_f64(rest, bone, weight, xforms):
    """every step in binary64 with the same formulas and this model's branches and flips, rounded once per step-4 float"""
    import _skin_dq_ref64 as R64
    info = {}
    skin_dq(rest, bone, weight, xforms, info)
    out, _, _ = R64.skin_dq(rest, bone, weight, xforms, info["branch"], info["flips"])
    with np.errstate(all="ignore"):
        return out.astype(f32).reshape(-1)


def skin_dq_fma(rest, bone, weight, xforms):
    """steps 1-3 as the rule has them, step 4 contracted as a compiler would: fma(m2, z, fma(m1, y, m0 * x)) + t (PM.pose_fma's chain)"""
    rest = np.ascontiguousarray(rest, f32).reshape(-1, 40)
    n = rest.shape[0]
    bone = np.asarray(bone, np.int64).reshape(-1, 4)
    B = corner_records(bone, np.ascontiguousarray(weight, f32).reshape(-1, 4), xforms)
    out = rest.copy()
    part = np.where(bone[:, 0] >= 0, np.arange(3 * n), -1).reshape(n, 3)
    for c in range(3):
        posed = PM.pose_fma(rest, part[:, c], B).reshape(n, 40)
        out[:, 4 * c:4 * c + 3] = posed[:, 4 * c:4 * c + 3]
        out[:, 12 + 4 * c:12 + 4 * c + 3] = posed[:, 12 + 4 * c:12 + 4 * c + 3]
    return out.reshape(-1)


# ---- shared cases

def rigid_records(n_parts, seed=5, shift=0.5, angles=None):
    """n_parts rigid records (rotation about a random axis by an angle in [0, 2 pi), a shift of the scene's scale; N = R), binary64 rounded once;
    the padding is NaN, which the rule ignores"""
    rng = np.random.RandomState(seed)
    M = []
    for k in range(n_parts):
        a = rng.uniform(0.0, 2.0 * np.pi) if angles is None else angles[k % len(angles)]
        M.append(PM.rotation(rng.normal(size=3), a, rng.uniform(-shift, shift, 3)))
    M = np.array(M).reshape(-1, 3, 4)
    X = PM.records(M, N=M[:, :, :3])
    X[:, 21:] = np.nan
    return X


def branch_records(seed=1):
    """eight rigid records, two per conversion branch: a small turn (the trace), then half turns and near-half turns about +x, +y, +z and axes near
    them (the largest diagonal is m00, m11, m22 in turn)"""
    rng = np.random.RandomState(seed)
    M = [PM.rotation((1, 2, 3), 0.3, (0.1, -0.2, 0.3)), PM.rotation((-1, 0.5, 0.2), 1.2, (0.0, 0.4, -0.1))]
    for axis in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        a = np.asarray(axis, np.float64)
        M.append(PM.rotation(a + 0.1 * rng.normal(size=3), np.pi - 0.05, rng.uniform(-0.5, 0.5, 3)))
        M.append(PM.rotation(a + 0.05 * rng.normal(size=3), np.pi + 0.4, rng.uniform(-0.5, 0.5, 3)))
    M = np.array(M).reshape(-1, 3, 4)
    X = PM.records(M, N=M[:, :, :3])
    X[:, 21:] = np.nan
    return X


def random_skin(n_tris, n_parts, seed=7, slots=None):
    """_skin_model.random_skin's tables (0-4 slots per corner mixed within a triangle, weights in [-0.5, 1.5], NaN in empty slots); slots: every
    moving corner has exactly that many, and every third corner is static"""
    import _skin_model as SM
    bone, weight = SM.random_skin(n_tris, n_parts, seed=seed)
    if slots is None or n_parts == 0:
        return bone, weight
    rng = np.random.RandomState(seed + 100)
    bone = rng.randint(0, n_parts, (3 * n_tris, 4)).astype(np.int32)
    weight = rng.uniform(-0.5, 1.5, (3 * n_tris, 4)).astype(f32)
    bone[:, slots:] = -1
    weight[:, slots:] = np.nan
    static = np.arange(3 * n_tris) % 3 == seed % 3
    if n_tris > 1:
        bone[static] = -1
        weight[static] = np.nan
    return bone.reshape(-1), weight.reshape(-1)


def dirichlet_skin(n_corners, n_parts, seed, static=0.0):
    """1-4 slots per corner, weights in [0, 1] that sum to 1 (rounded to binary32), NaN in the empty slots; a share `static` of the corners has none"""
    rng = np.random.RandomState(seed)
    count = rng.randint(1, 5, n_corners)
    count[rng.uniform(size=n_corners) < static] = 0
    bone = rng.randint(0, n_parts, (n_corners, 4)).astype(np.int32)
    weight = np.full((n_corners, 4), np.nan, f32)
    for k in range(0, 5):
        at = np.nonzero(count == k)[0]
        if k:
            weight[at, :k] = rng.dirichlet(np.ones(k), at.size)
        bone[at, k:] = -1
    return bone.reshape(-1), weight.reshape(-1)


def many_rigid_records(n_parts, seed=5, shift=0.5):
    """rigid_records for large tables, without a loop: rotations uniform over the sphere of unit quaternions (both signs of w: angles in
    [0, 2 pi)), binary64 rounded once"""
    rng = np.random.RandomState(seed)
    q = rng.normal(size=(n_parts, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    w, x, y, z = q.T
    M = np.zeros((n_parts, 3, 4))
    M[:, 0, :3] = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], axis=1)
    M[:, 1, :3] = np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], axis=1)
    M[:, 2, :3] = np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)
    M[:, :, 3] = rng.uniform(-shift, shift, (n_parts, 3))
    X = PM.records(M, N=M[:, :, :3])
    X[:, 21:] = np.nan
    return X
