"""CPU: the float32 model of include/pt_bloom.h (tests/_bloom_model.py), which tests/test_gpu_bloom.py holds the device to bit for bit — against the
float64 reference with its derived bound (tests/_bloom_ref64.py) on random images, against cases worked out by hand in this text, and against
what the rule promises: a one-colour image keeps its colour, an impulse keeps its sum, a mirror-symmetric image stays mirror symmetric exactly."""
import numpy as np
import pytest

import _bloom_model as BM
import _bloom_ref64 as R64
import _tonemap_model as TM

f32 = np.float32
U = 2.0 ** -24


def _image(pixels):
    """(c, A) of a list of (r, g, b, a) rows"""
    return TM.from_image(np.array(pixels, f32).reshape(-1, 4))


def _grey(values, a=1.0):
    """(c, A) of a 2-D array of grey values"""
    v = np.asarray(values, f32)
    img = np.stack([v, v, v, np.full(v.shape, a, f32)], -1)
    return TM.from_image(img)


# ---------------------------------------------------------------------------------------------------------------- against float64

@pytest.mark.parametrize("W,H,L,spread,thr", [(1, 1, 1, 1.0, 0.0), (2, 1, 2, 0.5, 0.0), (1, 7, 8, 1.0, 0.5), (5, 3, 8, 0.5, 0.0), (33, 17, 2, 0.75, 1.0),
                                              (64, 64, 6, 1.0, 0.0), (70, 37, 8, 0.5, 2.0), (70, 37, 1, 1.0, 0.0), (50, 27, 3, 0.3, 0.25)])
def test_the_model_is_within_the_derived_bound_of_float64(W, H, L, spread, thr):
    rs = np.random.RandomState(W * 131 + H * 7 + L)
    img = np.exp(rs.normal(-0.5, 2.0, (H, W, 4))).astype(f32)
    img[..., 3] = rs.randint(0, 4, (H, W))                           # some pixels emit nothing
    c, A = TM.from_image(img)
    for e in (1.0, 0.37):
        r = BM.rule(levels=L, spread=spread, threshold=thr, intensity=0.7)
        got = BM.bloom(c, A, W, H, r, e)
        ref, bound = R64.bloom(c, A, W, H, r, BM.threshold(thr, e))
        err = np.abs(got[..., :3].astype(np.float64) - ref[..., :3])
        assert (err <= bound).all(), (float((err / bound).max()), np.argwhere(err > bound)[:4].tolist())      # no pixel left out
        assert np.array_equal(got[..., 3], A.reshape(H, W))
        if L * thr == 0:
            assert err.max() > 0                                     # the two do differ: the bound is not met by being the same code


# ---------------------------------------------------------------------------------------------------------------- by hand

def test_a_1x1_image_by_hand():
    # every tap clamps to the one texel: a tent is (0.125p + 0.375p) + (0.375p + 0.125p) = p, up() is (0.5625p + 0.1875p) + (0.1875p + 0.0625p) = p
    c, A = _image([[2, 4, 8, 1]])
    out = BM.bloom(c, A, 1, 1, BM.rule(levels=1, threshold=0.0, intensity=0.5, spread=1.0), 1.0)
    assert out.tolist() == [[[3, 6, 12, 1]]]                         # threshold 0: k = (l - 0) / l = 1, G = c, out = c + 0.5 c
    # three levels, spread 0.5: U_3 = p, U_2 = p + 0.5p = 1.5p, U_1 = p + 0.5 * 1.5p = 1.75p; norm = 1 / ((1 + 0.5) + 0.25) = 1 / 1.75 rounded
    n = BM.norm(0.5, 3)
    assert n == f32(1.0) / f32(1.75) and BM.norm(1.0, 8) == f32(0.125) and BM.norm(0.3, 1) == 1
    out = BM.bloom(c, A, 1, 1, BM.rule(levels=3, threshold=0.0, intensity=1.0, spread=0.5), 1.0)
    assert out[0, 0].tolist() == [f32(2) + f32(3.5) * n, f32(4) + f32(7) * n, f32(8) + f32(14) * n, 1]
    # a threshold: c = (0, 4, 0) has l = 4 * 0.7152f exactly; T = 2 * 0.7152f (threshold 4 * 0.7152f under exposure 2): k = 0.5, B = (0, 2, 0)
    c, A = _image([[0, 4, 0, 3]])
    thr = float(f32(4) * f32(0.7152))
    assert BM.threshold(thr, 2.0) == f32(2) * f32(0.7152)
    out = BM.bloom(c, A, 1, 1, BM.rule(levels=1, threshold=thr, intensity=1.0, spread=1.0), 2.0)
    assert out.tolist() == [[[0, 6, 0, 3]]]
    # at the threshold and below it nothing blooms; a count of 0 or a NaN one emits nothing; a NaN channel stays, the others take the glare of the clean ones
    assert BM.bloom(c, A, 1, 1, BM.rule(levels=1, threshold=thr, intensity=1.0), 1.0).tolist() == [[[0, 4, 0, 3]]]
    for a in (0.0, -1.0, np.nan):
        c0, A0 = _image([[2, 4, 8, a]])
        assert BM.glare(c0, A0, 1, 1, BM.rule(levels=2, threshold=0.0), 1.0).tolist() == [[[0, 0, 0]]]
    cn, An = _image([[np.nan, 4, -8, 1]])                             # s = (0, 4, 0)
    out = BM.bloom(cn, An, 1, 1, BM.rule(levels=1, threshold=0.0, intensity=1.0), 1.0)[0, 0]
    assert np.isnan(out[0]) and out[1:].tolist() == [8, -8, 1]
    ci, Ai = _image([[np.inf, 0, 0, 1]])                              # s.r = 65504
    assert BM.glare(ci, Ai, 1, 1, BM.rule(levels=1, threshold=0.0), 1.0)[0, 0].tolist() == [65504, 0, 0]


def test_a_2x2_image_with_one_level_by_hand():
    # D_1 is 1 x 1: the taps clamp to columns 0, 0, 1, 1 and rows 0, 0, 1, 1, so a row is 0.5 p0 + 0.5 p1 and D_1 the mean of the four: 24.
    # up() of a 1 x 1 level is that texel everywhere: (13.5 + 4.5) + (4.5 + 1.5) = 24
    c, A = _grey([[8, 16], [24, 48]])
    r = BM.rule(levels=1, threshold=0.0, intensity=1.0, spread=1.0)
    assert BM.glare(c, A, 2, 2, r, 1.0).tolist() == [[[24] * 3] * 2] * 2
    assert BM.bloom(c, A, 2, 2, r, 1.0)[..., 0].tolist() == [[32, 40], [48, 72]]
    assert BM.sizes(2, 2, 3) == [(2, 2), (1, 1), (1, 1), (1, 1)] and BM.sizes(5, 3, 2) == [(5, 3), (3, 2), (2, 1)]


def test_an_impulse_in_a_4x4_image_with_two_levels_by_hand():
    # 4096 at (x, y) = (1, 1).  D_1 (2 x 2): output 0 reads columns 0, 0, 1, 2 — column 1 under weight 0.375 — and output 1 reads 1, 2, 3, 3 — under
    # 0.125; the same in y.  D_1 = 4096 * [[.375*.375, .125*.375], [.375*.125, .125*.125]] = [[576, 192], [192, 64]].
    # D_2 (1 x 1) = their mean = 256 = U_2.  spread 1: U_1 = D_1 + 256 = [[832, 448], [448, 320]], norm = 1/2.
    # up() to 4 x 4 weighs, per axis, texel (0, 1) by x = 0: (1, 0), 1: (.75, .25), 2: (.25, .75), 3: (0, 1).
    v = np.zeros((4, 4), f32)
    v[1, 1] = 4096
    c, A = _grey(v)
    r = BM.rule(levels=2, threshold=0.0, intensity=1.0, spread=1.0)
    B = BM.bright(BM.clean(c, A), 0.0)
    assert BM.down(B.reshape(4, 4, 3))[..., 1].tolist() == [[576, 192], [192, 64]]
    G = BM.glare(c, A, 4, 4, r, 1.0)[..., 0]
    assert G[0, 0] == 416 and G[3, 3] == 160 and G[0, 1] == 0.5 * (0.75 * 832 + 0.25 * 448) == 368
    assert G[1, 1] == 0.5 * ((468 + 84) + (84 + 20)) == 328
    axis = np.array([[1, 0], [.75, .25], [.25, .75], [0, 1]])
    U1 = np.array([[832, 448], [448, 320]], np.float64)
    assert np.array_equal(G, 0.5 * axis @ U1 @ axis.T)               # dyadic throughout: exact in both precisions
    assert G.sum() == 0.5 * 4 * (832 + 448 + 448 + 320) == 4096      # each axis' up() weights sum to 2 per texel: here the sum survives the borders


# ---------------------------------------------------------------------------------------------------------------- what the rule promises

@pytest.mark.parametrize("L,spread", [(1, 1.0), (3, 0.5), (6, 0.75), (8, 1.0), (8, 0.3)])
def test_a_one_colour_image_under_threshold_0_keeps_its_colour(L, spread):
    W, H = 37, 21
    colour = np.array([0.3, 1.7, 0.05], f32)
    img = np.empty((H, W, 4), f32)
    img[..., :3] = colour
    img[..., 3] = 2
    c, A = TM.from_image(img)
    G = BM.glare(c, A, W, H, BM.rule(levels=L, spread=spread, threshold=0.0), 1.0).astype(np.float64)
    bound = 1.01 * U * (13 * L + 9) * colour.astype(np.float64)      # _bloom_ref64's E_G with G64 = P(s) = the colour
    assert (np.abs(G - colour) <= bound).all(), (np.abs(G - colour) / bound).max()


@pytest.mark.parametrize("L,spread,thr", [(1, 1.0, 0.0), (3, 0.5, 0.0), (3, 1.0, 1.0)])
def test_an_impulse_away_from_the_borders_keeps_its_sum(L, spread, thr):
    W, H = 128, 96                                                   # the coarsest level is 16 x 12; the impulse lies 5 of its texels from every border
    v = np.zeros((H, W), f32)
    v[45, 61] = 1000.0
    c, A = _grey(v)
    r = BM.rule(levels=L, spread=spread, threshold=thr, intensity=1.0)
    G = BM.glare(c, A, W, H, r, 1.0).astype(np.float64)
    ref, bound = R64.bloom(c, A, W, H, r, BM.threshold(thr, 1.0))
    emitted = (ref[..., :3] - c.reshape(H, W, 3)).sum((0, 1))        # intensity 1: G64, summed
    s = BM.clean(c, A)[45 * W + 61].astype(np.float64)
    l = float(TM.luminance(s[None].astype(f32))[0])
    want = s * ((l - thr) / l)                                       # the impulse's B
    assert np.allclose(emitted, want, rtol=1e-6, atol=0)             # (its luminance is the float32 one here: 3u)
    assert (G[0] == 0).all() and (G[-1] == 0).all() and (G[:, 0] == 0).all() and (G[:, -1] == 0).all()      # nothing reached a border
    assert (np.abs(G.sum((0, 1)) - emitted) <= bound.sum((0, 1))).all()


def test_mirror_symmetry_is_exact():
    W = H = 64
    v = np.zeros((H, W), f32)
    for x, y, val in ((3, 5, 900.0), (20, 31, 77.5), (0, 0, 31.0), (31, 12, 5.25)):
        for xx in (x, W - 1 - x):
            for yy in (y, H - 1 - y):
                v[yy, xx] = val
    c, A = _grey(v)
    c[:, 0] *= f32(0.5)                                              # not a grey image
    for L, spread, thr in ((4, 0.5, 1.0), (6, 0.7, 0.0), (1, 1.0, 3.0)):
        G = BM.glare(c, A, W, H, BM.rule(levels=L, spread=spread, threshold=thr), 0.9)
        assert G.max() > 0
        assert np.array_equal(G, G[:, ::-1]) and np.array_equal(G, G[::-1])


def test_the_chain_with_the_tone_mapper():
    T = np.linspace(0, 1, 257)[:256].astype(f32)                     # any increasing table serves here
    rs = np.random.RandomState(5)
    W, H = 9, 6
    img = np.exp(rs.normal(0, 2, (H, W, 4))).astype(f32)
    c, A = TM.from_image(img)
    tm = TM.rule()
    plain = TM.tonemap(c, A, tm, T, W, H)
    zero = BM.tonemap_bloom(c, A, tm, BM.rule(intensity=0.0), T, W, H)
    lit = BM.tonemap_bloom(c, A, tm, BM.rule(intensity=0.5, threshold=0.0, levels=3), T, W, H)
    for got in (zero, lit):
        assert got[1] == plain[1] and np.array_equal(got[2], plain[2])      # the metering is the source's
    assert np.array_equal(zero[0], plain[0]) and (lit[0].astype(int) >= plain[0].astype(int)).all() and (lit[0] != plain[0]).any()
