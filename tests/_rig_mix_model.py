"""include/pt_rig_mix.h's rule in numpy binary32, written from the header and not from the C++: every array is float32 and every numpy operation
rounds once, so a * b + c below is a rounded product and a rounded sum, in the order written.  The key blend, the interval and the records are
tests/_rig_model.py's (include/pt_rig.h), imported and not copied.  Also the cases the mix's tests share."""
import numpy as np

import _rig_model as RM

f32 = np.float32
SLOTS, MASKS, MAX_LAYERS = 16, 8, 8
OVERRIDE, ADDITIVE = 0, 1
CLAMP, LOOP = 0, 1


def layer(clip, t, weight=1.0, mask=-1, mode=OVERRIDE, wrap=CLAMP):
    return dict(clip=int(clip), t=f32(t), weight=f32(weight), mask=int(mask), mode=int(mode), wrap=int(wrap))


def wrap_time(times, t):
    """step 1, the loop wrap of a finite t into a clip of more than one key"""
    T = np.ascontiguousarray(times, f32)
    D = f32(T[-1] - T[0])
    x = f32(f32(t) - T[0])
    r = f32(np.fmod(x, D))                                            # exact
    if r < 0:
        r = f32(r + D)
    return f32(T[0] + r)


def step(times, wrap, t):
    """step 1: (ka, kb, u) of a layer; at a key, or clamped, ka == kb and u == 0"""
    T = np.ascontiguousarray(times, f32)
    if T.size == 1:
        return 0, 0, f32(0)
    t = f32(t)
    if wrap == LOOP:
        t = wrap_time(T, t)
    exact, k, u = RM.interval(T, t)
    return (exact, exact, f32(0)) if exact >= 0 else (k, k + 1, u)


def qmul(p, q):
    """p (x) q on (n, 4) arrays of (x y z w), in the header's order"""
    px, py, pz, pw = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    qx, qy, qz, qw = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    w = ((pw * qw - px * qx) - py * qy) - pz * qz
    x = ((pw * qx + px * qw) + py * qz) - pz * qy
    y = ((pw * qy - px * qz) + py * qw) + pz * qx
    z = ((pw * qz + px * qy) - py * qx) + pz * qw
    return np.stack([x, y, z, w], axis=1).astype(f32)


def blend_each(a, b, e):
    """RM.blend with a weight per joint (none of them 0 or 1): the joints of each distinct weight go through it together"""
    out = np.zeros_like(a)
    for ev in np.unique(e):
        js = e == ev
        out[js] = RM.blend(a[js], b[js], ev)
    return out


def mix_locals(clips, masks, layers, n, trace=None):
    """steps 1-7: (n, 12) float32.  clips: {slot: (times, values)}, masks: {slot: weights}, layers: a list of layer(...).  trace, a list, receives
    per layer what the rule decided: dict(ka, kb, u, e, key_flip, flip, neg), arrays per joint where they are per joint"""
    acc = None
    with np.errstate(all="ignore"):
        for l, y in enumerate(layers):
            times, values = clips[y["clip"]]
            V = np.ascontiguousarray(values, f32).reshape(len(times), n, 12)
            ka, kb, u = step(times, y["wrap"], y["t"])
            S = V[ka].copy() if u == 0 else RM.blend(V[ka], V[kb], u)                  # step 2
            seen = dict(ka=ka, kb=kb, u=u, key_flip=RM.flips(V[ka], V[kb]) if u != 0 else np.zeros(n, bool))
            if trace is not None:
                trace.append(seen)
            if l == 0:                                                               # step 4
                acc = S.copy()
                continue
            w = f32(y["weight"])
            e = np.full(n, w, f32) if y["mask"] < 0 else (w * np.ascontiguousarray(masks[y["mask"]], f32)).astype(f32)      # step 3
            seen["e"] = e
            part = (e != 0) & (e != 1)
            new = acc.copy()
            if y["mode"] == OVERRIDE:                                                # step 5
                new[e == 1] = S[e == 1]
                new[part] = blend_each(acc[part], S[part], e[part])
                seen["flip"] = RM.flips(acc, S)
            else:                                                                    # step 6
                R = V[0]
                ec = e[:, None]
                moved = acc + ec * (S - R)
                conj = np.concatenate([-R[:, 4:7], R[:, 7:8]], axis=1)
                dq = qmul(S[:, 4:8], conj)
                neg = dq[:, 3] < 0
                dq[neg] = -dq[neg]
                v = f32(1.0) - e
                dp = np.stack([e * dq[:, 0], e * dq[:, 1], e * dq[:, 2], v + e * dq[:, 3]], axis=1).astype(f32)
                moved[:, 4:8] = qmul(dp, acc[:, 4:8])
                new[e != 0] = moved[e != 0]
                seen["neg"] = neg
            acc = new
    out = acc.copy()
    out[:, 3] = out[:, 11] = 0                                                       # step 7
    return out


def mix_records(parent, clips, masks, layers, inv_bind=None):
    n = np.asarray(parent).size
    return RM.records(parent, mix_locals(clips, masks, layers, n), inv_bind)


# ------------------------------------------------------------------------------------------------ the cases

JOINTS = (0, 1, 2, 65, 255, 256, 257, 1000)      # one block, its edge, one lane into a second; a wave and a lane; nothing at all
TIMES4 = np.array([0.25, 1.0, 1.5, 4.0], f32)
TIMES2 = np.array([0.0, 2.0], f32)


def ramp(n):
    return (np.arange(n, dtype=np.float64) / max(n - 1, 1)).astype(f32)


def slots(n, seed=0):
    """the clips and masks of a case: slot 0 four keys of unnormalised q, slot 3 two keys of unit q, slot 15 one key; masks 0: all 0, 1: all 1,
    7: a ramp from 0 to 1.  The paddings hold NaN: they are never read"""
    clips = {0: (TIMES4, np.stack([RM.random_locals(n, seed + 20 + k) for k in range(4)])),
             3: (TIMES2, np.stack([RM.random_locals(n, seed + 30 + k, unnormalised=False) for k in range(2)])),
             15: (np.array([2.0], f32), RM.random_locals(n, seed + 40, unnormalised=False)[None])}
    masks = {0: np.zeros(n, f32), 1: np.ones(n, f32), 7: ramp(n)}
    return clips, masks


LAYER_SETS = {
    "one": [layer(0, 1.125)],
    "one at a key": [layer(0, 1.0)],
    "one looped": [layer(0, 5.0, wrap=LOOP)],
    "two": [layer(0, 0.5), layer(3, 2.75, 0.625, 7, OVERRIDE, LOOP)],
    # both modes, both wraps, the three masks and none, slots shared, layers at a key (u == 0) and between keys
    "eight": [layer(0, 1.25), layer(3, 0.5, 0.5), layer(3, 2.0, 0.75, 7, ADDITIVE), layer(0, -1.0, 1.0, 0, OVERRIDE, LOOP), layer(15, 9.0, 0.25, 1, ADDITIVE, LOOP),
              layer(0, 6.5, 1.0, 7, OVERRIDE, LOOP), layer(3, 1.0, 1.0, 1, OVERRIDE), layer(0, 3.0, 0.3, 7, ADDITIVE, CLAMP)],
    "eight at keys": [layer(0, 0.25), layer(3, 2.0, 0.5), layer(3, 0.0, 0.75, 7, ADDITIVE), layer(0, 1.5, 1.0, 0), layer(15, 0.0, 0.25, 1, ADDITIVE),
                      layer(0, 4.0 + 3.75 * 2, 0.5, 7, OVERRIDE, LOOP), layer(3, -5.0, 1.0, 7), layer(0, 9.0, 0.3, -1, ADDITIVE)],
    "eight between keys": [layer(0, 0.5), layer(3, 0.5, 0.5), layer(3, 1.75, 0.75, 7, ADDITIVE), layer(0, 2.0, 1.0, 0), layer(0, 1.125, 0.25, 1, ADDITIVE),
                           layer(0, 6.5, 0.5, 7, OVERRIDE, LOOP), layer(3, 0.125, 1.0, 7), layer(0, 3.0, 0.3, -1, ADDITIVE)],
}


def mix_cases():
    """(tag, n, clips, masks, layers): every joint count under the eight mixed layers and under two, and every set of layers at 65 and 257"""
    out = []
    for n in JOINTS:
        clips, masks = slots(n)
        for name, layers in LAYER_SETS.items():
            if name in ("eight", "two") or n in (65, 257):
                out.append(((f"n{n}", name), n, clips, masks, layers))
    return out
