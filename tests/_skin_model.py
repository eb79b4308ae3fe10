"""The rule of include/pt_skin.h in numpy binary32: per corner the blend of up to four records, every product rounded before every sum in slot
order, then tests/_pose_model.py's arithmetic (PM.pose with one "part" per corner) on the blended record.  Also the two blends the rule is NOT (in
binary64 rounded once, and fused), so that a test can show the comparison tells them apart, and the cases the CPU and GPU tests share."""
import numpy as np

import _pose_model as PM

f32 = np.float32
REC = PM.REC


def blend(bone, weight, xforms):
    """bone, weight: (n_corners, 4); xforms: records of 24 floats -> (n_corners, 24) blended records (rows of static corners: zero)"""
    bone = np.asarray(bone, np.int64).reshape(-1, 4)
    w = np.ascontiguousarray(weight, f32).reshape(-1, 4)
    X = np.ascontiguousarray(xforms, f32).reshape(-1, REC)
    B = np.zeros((bone.shape[0], REC), f32)
    with np.errstate(all="ignore"):
        for s in range(4):
            use = np.nonzero(bone[:, s] >= 0)[0]
            if use.size == 0:
                continue
            p = (w[use, s, None] * X[bone[use, s], :21]).astype(f32)
            B[use, :21] = p if s == 0 else (B[use, :21] + p).astype(f32)
    return B


def blend_f64(bone, weight, xforms):
    """what the blend is not: the sum in binary64, rounded once"""
    bone = np.asarray(bone, np.int64).reshape(-1, 4)
    w = np.ascontiguousarray(weight, f32).reshape(-1, 4).astype(np.float64)
    X = np.ascontiguousarray(xforms, f32).reshape(-1, REC).astype(np.float64)
    B = np.zeros((bone.shape[0], REC), np.float64)
    for s in range(4):
        use = np.nonzero(bone[:, s] >= 0)[0]
        B[use, :21] += w[use, s, None] * X[bone[use, s], :21]
    return B.astype(f32)


def blend_fma(bone, weight, xforms):
    """what the blend is not: B = fma(w_s, x_s, B), the chain a compiler contracts it to"""
    bone = np.asarray(bone, np.int64).reshape(-1, 4)
    w = np.ascontiguousarray(weight, f32).reshape(-1, 4)
    X = np.ascontiguousarray(xforms, f32).reshape(-1, REC)
    B = np.zeros((bone.shape[0], REC), f32)
    for k in range(bone.shape[0]):
        for j in range(21):
            for s in range(4):
                if bone[k, s] < 0:
                    break
                x = X[bone[k, s], j]
                B[k, j] = f32(w[k, s] * x) if s == 0 else PM._fma(w[k, s], x, B[k, j])
    return B


def skin(rest, bone, weight, xforms, blender=blend):
    """rest: 40 floats per triangle; bone, weight: 12 per triangle -> the posed binding 3"""
    rest = np.ascontiguousarray(rest, f32).reshape(-1, 40)
    n = rest.shape[0]
    bone = np.asarray(bone, np.int64).reshape(n, 3, 4)
    out = rest.copy()
    if n == 0:
        return out.reshape(-1)
    B = blender(bone.reshape(-1, 4), np.ascontiguousarray(weight, f32).reshape(-1, 4), xforms)      # one record per corner
    part = np.where(bone[:, :, 0].reshape(-1) >= 0, np.arange(3 * n), -1)
    for c in range(3):
        # PM.pose on triangles of which only corner c's two float4 are kept: "triangle" k under "part" 3k + c
        posed = PM.pose(rest, part.reshape(n, 3)[:, c], B).reshape(n, 40)
        out[:, 4 * c:4 * c + 3] = posed[:, 4 * c:4 * c + 3]
        out[:, 12 + 4 * c:12 + 4 * c + 3] = posed[:, 12 + 4 * c:12 + 4 * c + 3]
    return out.reshape(-1)


def skin_of_parts(tri_part):
    """the single-slot weight-1 skin of a part table: (bone, weight), 12 per triangle"""
    part = np.asarray(tri_part, np.int32).reshape(-1)
    bone = np.full((part.size, 3, 4), -1, np.int32)
    bone[:, :, 0] = part[:, None]
    weight = np.zeros((part.size, 3, 4), f32)
    weight[:, :, 0] = 1.0
    return bone.reshape(-1), weight.reshape(-1)


def random_skin(n_tris, n_parts, seed=7, top_bone=False):
    """0-4 slots per corner, mixed within a triangle (so static corners lie inside moving triangles); weights in [-0.5, 1.5], those of empty
    slots NaN; top_bone: bone n_parts - 1 is used by the first corner that has a slot"""
    rng = np.random.RandomState(seed)
    count = rng.randint(0, 5, (n_tris, 3))
    if n_parts == 0:
        count[:] = 0
    bone = rng.randint(0, max(n_parts, 1), (n_tris, 3, 4)).astype(np.int32)
    weight = rng.uniform(-0.5, 1.5, (n_tris, 3, 4)).astype(f32)
    empty = np.arange(4)[None, None, :] >= count[:, :, None]
    bone[empty] = -1
    weight[empty] = np.nan
    if top_bone and (count > 0).any():
        k, c = np.argwhere(count > 0)[0]
        bone[k, c, 0] = n_parts - 1
    return bone.reshape(-1), weight.reshape(-1)


def shared_corners_crack(tris, bone, weight, rest):
    """the number of corner pairs with equal rest floats (vertex and normal) and equal skin words whose posed floats differ in a bit"""
    rest = np.ascontiguousarray(rest, f32).reshape(-1, 40).view(np.uint32)
    out = np.ascontiguousarray(tris, f32).reshape(-1, 40).view(np.uint32)
    n = rest.shape[0]
    b = np.asarray(bone, np.int32).reshape(n, 3, 4).view(np.uint32)
    w = np.ascontiguousarray(weight, f32).reshape(n, 3, 4).view(np.uint32)
    seen, cracks, shared = {}, 0, 0
    for k in range(n):
        for c in range(3):
            key = (rest[k, 4 * c:4 * c + 3].tobytes(), rest[k, 12 + 4 * c:15 + 4 * c].tobytes(), b[k, c].tobytes(), w[k, c].tobytes())
            got = (out[k, 4 * c:4 * c + 3].tobytes(), out[k, 12 + 4 * c:15 + 4 * c].tobytes())
            if key in seen:
                shared += 1
                cracks += seen[key] != got
            else:
                seen[key] = got
    return cracks, shared
