"""GPU: seen-through feature records (include/pt_through.h).  Every recorded surface against the oracle's rayScene along the segment that
pt_read_through_rays reports; the chain against the float32 model of tests/_through_model.py; depth 0 bit for bit against the first-hit calls;
the fill and the filter on the device's own records against tests/_fill_model.py; across context kinds, the cache, FRAME, and at 1080p."""
import ctypes as C

import numpy as np
import pytest

import _through_model as TM
from _fill_model import denoise_guided_filled as model
from _fill_model import fill_frame
from test_gpu_fill import OFF, REAL, SAFE, _holes
from test_gpu_guided import _inject

pytestmark = pytest.mark.gpu

W, H = 48, 27
NPIX = 400                                          # the subsets of tests/test_gpu_features.py (same seeds: the scene's index in its list)
INF = float("inf")
BOTH = TM.REFLECT | TM.TRANSMIT
SCENES = [("C1", 0), ("C3", 2), ("C5", 4), ("C6", 5), ("T1", 6)]
f32 = np.float32


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.int32)


def _i(x):
    return int(np.float32(x).view(np.int32))


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


def _open(pt, renderer_mod, scene, w=W, h=H, wl=None, options=None, **kw):
    """options: pt_set_option names and values, set before the scene is loaded (index_stack_8bit: the encoding of the index stack)"""
    wl = pt.scenes.build(scene, w, h) if wl is None else wl
    r = renderer_mod.Renderer(w, h, **kw)
    for k, v in (options or {}).items():
        r.set_option(k, v)
    r.load_workload(wl)
    return r, wl


def _rule(r, depth=4, min_weight=0.5, lobes=BOTH, key=True):
    return r.through_rule(depth, min_weight, lobes, key)


@pytest.mark.parametrize("scene,seed", SCENES)
def test_recorded_surfaces_match_the_oracle(pt, oracle, renderer_mod, scene, seed):
    """rayScene along the reported segment reproduces the record's hit code, the segment's t and the material bit for bit, and N where the
    material has no map_norm"""
    w, h = (48, 48) if scene == "C1" else (W, H)
    r, wl = _open(pt, renderer_mod, scene, w, h)
    rule = _rule(r)
    feat, rays = r.read_features_through(rule).reshape(-1, 16), r.read_through_rays(rule).reshape(-1, 8)
    first = r.read_features().reshape(-1, 16)
    r.close()
    mats = TM.materials(wl.buffers[14])
    sc = oracle.Scene.from_workload(wl)
    k = _i32(feat[:, 14])
    assert np.array_equal(k, _i32(rays[:, 7])) and k.min() >= 0 and k.max() <= 4
    assert _bits_equal(feat[:, 8:11], first[:, 8:11])                        # D0 stays the lens-centre direction
    assert _bits_equal(feat[k == 0], first[k == 0])                           # no step taken: the first-hit record
    assert _bits_equal(rays[k == 0][:, 4:7], first[k == 0][:, 8:11]) and _bits_equal(rays[k == 0][:, 3], first[k == 0][:, 0])
    pix = np.random.RandomState(seed).choice(w * h, size=min(NPIX, w * h), replace=False)
    for p in pix:
        rec, ry = feat[p], rays[p]
        code, out = oracle.ray_scene(sc, ry[0:3], ry[4:7])
        code = int(code) if code >= 0 else -1
        assert _i(rec[7]) == code, (scene, p, _i(rec[7]), code)
        assert _i(ry[3]) == _i(out[0]), (scene, p, ry[3], out[0])
        if code < 0:
            assert k[p] == 0 and ry[3] == -1 and _i(rec[11]) == -1
            continue
        mat = _i(rec[11]) & 0xFFF if k[p] > 0 else _i(rec[11])
        assert mat == int(out[7]), (scene, p, mat, out[7])
        if k[p] > 0:
            assert _i(rec[11]) == (int(k[p]) << 24) | (_i(first[p][11]) << 12) | mat
        if mats[mat][37] <= -1:
            assert np.array_equal(rec[1:4], out[4:7], equal_nan=True), (scene, p, rec[1:4], out[4:7])


def _against_model(pt, oracle, renderer_mod, scene, rule_args, wl=None, stack=0, records=None):
    """the device's records and rays of a scene under a rule against the model's; returns how many pixels the model follows.
    stack: pt_set_option index_stack_8bit (0 the scene's own encoding, 1 8-bit codes, 2 the ten floats).  records: a list that takes (feat, rays)."""
    w, h = (48, 48) if scene == "C1" else (W, H)
    r, wl = _open(pt, renderer_mod, scene, w, h, wl=wl, options={"index_stack_8bit": stack})
    rule = _rule(r, *rule_args)
    feat, rays = r.read_features_through(rule), r.read_through_rays(rule)
    r.close()
    if records is not None:
        records.append((feat, rays))
    depth, mw, lobes, key = rule_args
    want, wrays, info = TM.through_features(oracle, wl, feat[..., 8:11], depth, mw, lobes, TM.KEY if key else 0, uv=True, fragile=True)
    mk = _i32(want[..., 14])
    followed = mk > 0
    skip = info["fragile"]
    print(f"{scene} {rule_args}: followed {int(followed.sum())} of {w * h} (by k {np.bincount(mk.ravel(), minlength=depth + 1).tolist()}), "
          f"fragile {int(skip.sum())}, of them followed {int((skip & followed).sum())}")
    assert (skip & followed).sum() <= 0.01 * followed.sum(), (scene, int(skip.sum()), int(followed.sum()))
    ok = ~skip
    assert np.array_equal(_i32(feat[..., 14])[ok], mk[ok])
    assert np.array_equal(_i32(feat[..., 11])[ok], _i32(want[..., 11])[ok])
    assert np.array_equal(_i32(feat[..., 7])[ok], _i32(want[..., 7])[ok])
    hit = ok & (_i32(want[..., 7]) >= 0)
    assert np.allclose(feat[..., 0][hit], want[..., 0][hit], rtol=1e-5, atol=0)
    assert np.abs(rays[..., 4:7][ok] - wrays[..., 4:7][ok]).max() < 1e-6
    # S1 = tint * Kd in chain order and S3's uv: the model's operations are the device's, so bit for bit; where texels enter (T1) the model's
    # bilinear filter is held to 1e-6 relative instead.
    # An ellipsoid inherits the uv of the closest triangle found before it, which the model does not trace: triangle hits only.
    tri = hit & ((_i32(want[..., 7]) >> 24) == 1)
    if getattr(wl, "textures", None):
        assert np.allclose(feat[..., 4:7][hit], want[..., 4:7][hit], rtol=1e-6, atol=1e-7)
        assert np.allclose(feat[..., 12:14][tri], want[..., 12:14][tri], rtol=1e-6, atol=1e-6)
    else:
        assert _bits_equal(feat[..., 4:7][hit], want[..., 4:7][hit])
        assert _bits_equal(feat[..., 12:14][tri], want[..., 12:14][tri])
    return int(followed.sum())


@pytest.mark.parametrize("scene", [s for s, _ in SCENES])
def test_chain_agrees_with_the_float32_model(pt, oracle, renderer_mod, scene):
    """k, the surface word and the hit code equal the model's; L within rtol 1e-5; the last direction within 1e-6 absolute (the bound of the
    direction test of tests/test_gpu_features.py).  The model starts from the device's own D0.  A pixel is left out where the model's own
    decision is fragile (a weight within 1e-5 of a threshold of step 6, or a chain that changes when the directions are recomputed in float64
    and rounded), at most 1 % of the followed pixels.  The model alone, on these scenes with rule (4, 0.5, both, KEY), along the float64 camera
    model's directions: C1 0 fragile of 12 followed (2304 pixels), C3 0 of 155, C5 0 of 28, C6 0 of 196, T1 0 of 0 (1296 pixels each)."""
    n = _against_model(pt, oracle, renderer_mod, scene, (4, 0.5, BOTH, True))
    assert n > 0 or scene == "T1"                     # T1's mapped box never reaches a weight of 0.5: see the next test


@pytest.mark.parametrize("rule_args", [(4, 0.3, BOTH, True), (2, 0.3, TM.REFLECT, False)])
def test_chain_through_mapped_materials(pt, oracle, renderer_mod, rule_args):
    """T1 at a min_weight its box with map_Pr / map_Pm / map_Pc / map_Tr reaches: the weights come from texels at the hit's uv"""
    assert _against_model(pt, oracle, renderer_mod, "T1", rule_args) > 0


def test_rules_other_than_the_default(pt, oracle, renderer_mod):
    for rule_args in ((4, 0.8, TM.REFLECT, True), (4, 0.8, TM.REFLECT, False), (1, 0.5, TM.TRANSMIT, True), (8, 0.5, BOTH, True)):
        assert _against_model(pt, oracle, renderer_mod, "C3", rule_args) > 0


@pytest.mark.parametrize("scene", ["C3", "C6"])
def test_every_index_stack_encoding_gives_the_same_chains(pt, oracle, renderer_mod, scene):
    """k_through_step<3>, <8> and <32> (pt_set_option index_stack_8bit 0, 1, 2, as tests/test_gpu_parity.py switches k_shade's): both lobes at
    depth 4 push and pop the stack through the glass.  Each agrees with the model, and the records and rays are bit-identical across the three."""
    got = []
    for stack in (0, 1, 2):
        assert _against_model(pt, oracle, renderer_mod, scene, (4, 0.5, BOTH, True), stack=stack, records=got) > 100
    for feat, rays in got[1:]:
        assert _bits_equal(feat, got[0][0]) and _bits_equal(rays, got[0][1])
    # the same at a size where thousands of pixels pass through glass, and the fill on them
    big = []
    for stack in (0, 1, 2):
        r, _ = _open(pt, renderer_mod, scene, 192, 108, options={"index_stack_8bit": stack})
        rule = _rule(r)
        big.append((r.read_features_through(rule), r.read_through_rays(rule), r.read_features()))
        r.close()
    assert (_i32(big[0][0][..., 14]) >= 2).sum() > 500
    for rec in big[1:]:
        assert all(_bits_equal(a, b) for a, b in zip(rec, big[0]))


def test_a_nan_normal_stops_the_chain_at_step_seven(pt, oracle, renderer_mod):
    """cubes without vertex normals (NaN normals) made polished metal: the weights do not read N, so reflection is chosen with
    r' = 1 and reflect(D, N) is NaN: step 7 stops the chain on the cube.  The ground has normals and the same metal: its chains go on."""
    from test_gpu_parity import _no_vn_workload
    base = _no_vn_workload(pt, W, H)
    m = np.array(base.buffers[14], f32)
    m[25], m[26] = 1.0, 0.0                            # material 0: Pm 1, Pr 0
    b = dict(base.buffers); b[14] = m
    wl = pt.scenes.Workload("no_vn_metal", W, H, b, base.sky, base.sample_res, base.max_bounces, base.info)
    got = []
    assert _against_model(pt, oracle, renderer_mod, "no_vn_metal", (4, 0.8, TM.REFLECT, True), wl=wl, records=got) > 0
    feat = got[0][0]
    nan = np.isnan(feat[..., 1:4]).any(-1) & (_i32(feat[..., 14]) == 0)
    assert nan.sum() > 20                               # cubes seen directly: stopped at k = 0 with their NaN normal in the record


@pytest.mark.parametrize("scene", ["C3", "T1", "C6"])
def test_depth_zero_is_the_first_hit_path_bit_for_bit(pt, renderer_mod, scene):
    r, _ = _open(pt, renderer_mod, scene, 96, 54)
    first = r.read_features()
    fr, T, _ = _holes(*_inject(first))
    r.write_frame(fr)
    r.write_moments(T)
    for rule in (_rule(r, 0), _rule(r, 4, 0.5, 0), _rule(r, 0, 1.0, TM.REFLECT, False)):
        assert _bits_equal(r.read_features_through(rule), first)
        rays = r.read_through_rays(rule)
        assert _bits_equal(rays[..., 3], first[..., 0]) and _bits_equal(rays[..., 4:7], first[..., 8:11]) and not _i32(rays[..., 7]).any()
        for floor in (None, 0.2):
            a, na = r.fill_frame(*REAL, albedo_floor=floor)
            b, nb = r.fill_frame(*REAL, albedo_floor=floor, through=rule)
            assert na == nb and _bits_equal(a, b)
            a = r.denoise_guided(5, 2.0, *REAL, min_frames=4, albedo_floor=floor, fill=True)
            b = r.denoise_guided(5, 2.0, *REAL, min_frames=4, albedo_floor=floor, fill=True, through=rule)
            assert _bits_equal(a, b)
            a = r.read_display_denoised_guided(5, 2.0, *REAL, min_frames=4, albedo_floor=floor, fill=True)
            b = r.read_display_denoised_guided(5, 2.0, *REAL, min_frames=4, albedo_floor=floor, fill=True, through=rule)
            assert np.array_equal(a, b)
    r.close()


def test_raytracing_off_takes_no_step(pt, renderer_mod):
    wl = pt.scenes.build("C3", 96, 54).with_params(RAYTRACING=0)
    r = renderer_mod.Renderer(96, 54)
    r.load_workload(wl)
    assert _bits_equal(r.read_features_through(_rule(r)), r.read_features())
    r.close()


# (scene, the fill's sigmas).  n_filled is exact only where no tap weight lies at the fill's 1e-30 cut, which the test asserts from the model
# (a factor 100 either side).  SAFE and OFF keep every weight away from it by construction (tests/test_gpu_fill.py); REAL, the renderer's
# default, does so on C3's records.  On C6's its depth term, now over whole chains' lengths, puts one weight within 0.6 % of the cut, so C6
# runs SAFE and OFF.
FILL_CASES = [("C3", (REAL, SAFE)), ("C6", (SAFE, OFF))]


@pytest.mark.parametrize("scene,geos", FILL_CASES)
def test_fill_and_filter_at_depth_four_match_the_model(pt, renderer_mod, scene, geos):
    """the fill and the filter kernels run unchanged on the through buffer: device output against tests/_fill_model.py on the device's own S"""
    r, _ = _open(pt, renderer_mod, scene, 96, 54)
    rule = _rule(r)
    S = r.read_features_through(rule)
    assert (_i32(S[..., 14]) > 0).sum() > 50 and not _bits_equal(S, r.read_features())
    fr, T, hole = _holes(*_inject(S))
    r.write_frame(fr)
    r.write_moments(T)
    for geo in geos:
        for floor in (0.0, 0.2):
            got, n = r.fill_frame(*geo, albedo_floor=floor if floor else None, through=rule)
            want, wn, d = fill_frame(fr, S, *geo, floor, detail=True)
            print(scene, geo, floor, "filled", n, "margin", float(d["margin"].min()))
            assert d["margin"].min() >= 100.0, (geo, floor, float(d["margin"].min()))      # no weight near the cut: the count cannot pass by luck
            assert n == wn, (geo, floor, n, wn)
            assert np.allclose(got, want, rtol=1e-4, atol=1e-6, equal_nan=True), (geo, floor, np.nanmax(np.abs(got - want)))
            assert _bits_equal(got[~d["filled"]], fr[~d["filled"]])
    for it, lum_sigma, geo, mf in ((5, 2.0, geos[0], 4), (3, 1.0, geos[1], 2), (0, 2.0, geos[0], 4)):
        for floor in (0.0, 0.2):
            got = r.denoise_guided(it, lum_sigma, *geo, min_frames=mf, albedo_floor=floor if floor else None, fill=True, through=rule)
            want = model(fr, S, T, it, lum_sigma, *geo, mf, floor)
            assert np.allclose(got, want, rtol=1e-4, atol=1e-6, equal_nan=True), (scene, it, geo, mf, floor, np.nanmax(np.abs(got - want)))
            assert np.array_equal(got[..., 3], fr[..., 3])
            disp = r.read_display_denoised_guided(it, lum_sigma, *geo, min_frames=mf, albedo_floor=floor if floor else None, fill=True, through=rule,
                                                  java_bytes=False)
            q = np.floor(np.clip(np.nan_to_num(got[::-1, :, :3], nan=0.0), 0, 1) * f32(255) + f32(0.5)).astype(np.uint8)
            assert np.array_equal(disp, q)
    assert _bits_equal(r.read_frame(), fr) and _bits_equal(r.read_moments(), T)
    r.close()


@pytest.mark.parametrize("kind", ["sharded", "multi_stream", "virtual_multi"])
def test_every_context_gives_the_same_records(pt, renderer_mod, monkeypatch, kind):
    def records(**ctx):
        r, _ = _open(pt, renderer_mod, "C3", 96, 54, **ctx)
        out = r.read_features_through(_rule(r)), r.read_through_rays(_rule(r))
        r.close()
        return out
    ref = records()
    if kind == "sharded":
        got = records(shard_rank=1, shard_count=3)
    elif kind == "multi_stream":
        got = records(devices=[0, 0])
    else:
        monkeypatch.setenv("PT_MULTI_VIRTUAL_DEVICES", "2")
        got = records(devices=[0, 0])
    assert _bits_equal(got[0], ref[0]) and _bits_equal(got[1], ref[1])


def test_camera_and_rule_changes_recompute(pt, renderer_mod):
    wl = pt.scenes.build("C3", 96, 54)
    r = renderer_mod.Renderer(96, 54)
    r.load_workload(wl)
    deep, shallow = _rule(r), _rule(r, 1)
    r.set_timing(True)                                                          # the intersect launches of a probe pool are counted
    launches = lambda: r.kernel_time("extend")[0]                               # noqa: E731
    n0 = launches()
    a = r.read_features_through(deep)
    n1 = launches()
    assert n1 > n0                                                              # max_depth + 1 rounds
    assert _bits_equal(r.read_features_through(deep), a) and launches() == n1   # reused: nothing launched
    r.read_through_rays(deep)
    r.fill_frame(through=deep)
    assert launches() == n1                                                     # ... by the other calls too
    b = r.read_features_through(shallow)
    assert 0 < launches() - n1 < n1 - n0                                        # a changed rule recomputes, in fewer rounds at depth 1
    assert not _bits_equal(a, b) and _i32(b[..., 14]).max() == 1 and _i32(a[..., 14]).max() > 1
    assert _bits_equal(r.read_features_through(deep), a)                        # the rule changed back: recomputed
    nokey = r.read_features_through(_rule(r, key=False))
    assert not _bits_equal(nokey[..., 11], a[..., 11]) and _bits_equal(nokey[..., :11], a[..., :11])
    cam = np.asarray(wl.buffers[0], f32) + f32(0.2)
    r.set_buffer(0, cam)
    moved = r.read_features_through(deep)
    r.close()
    b2 = dict(wl.buffers); b2[0] = cam
    fresh = renderer_mod.Renderer(96, 54)
    fresh.load_workload(pt.scenes.Workload("C3_moved", 96, 54, b2, wl.sky, wl.sample_res, wl.max_bounces, wl.info))
    want = fresh.read_features_through(_rule(fresh))
    fresh.close()
    assert not _bits_equal(a, moved) and _bits_equal(moved, want)


def test_through_calls_between_renders_leave_frame_bit_identical(pt, renderer_mod):
    wl = pt.scenes.build("C3", 96, 54)
    seeds = [pt.scenes.frame_seed(f) for f in range(1, 5)]
    imgs = []
    for probe in (False, True):
        r = renderer_mod.Renderer(96, 54)
        r.load_workload(wl)
        r.record_moments()
        r.render_batch(1, seeds[:2])
        if probe:
            r.read_features_through(_rule(r))
            r.fill_frame(through=_rule(r, 2))
        r.render_batch_async(3, seeds[2:])
        if probe:
            r.read_through_rays(_rule(r, 3))
            r.denoise_guided(fill=True, through=_rule(r))
        imgs.append((r.read_frame(), r.read_moments()))
        r.close()
    assert _bits_equal(imgs[0][0], imgs[1][0]) and _bits_equal(imgs[0][1], imgs[1][1])


def test_full_size_c3_last_segments_equal_debug_intersect(pt, renderer_mod):
    r, _ = _open(pt, renderer_mod, "C3", 1920, 1080)
    rule = _rule(r)
    f = r.read_features_through(rule).reshape(-1, 16)
    rays = r.read_through_rays(rule).reshape(-1, 8)
    tuv, prim = r.debug_intersect(np.ascontiguousarray(rays[:, 0:3]), np.ascontiguousarray(rays[:, 4:7]))
    r.close()
    hit = _i32(f[:, 7]) >= 0
    code = np.where(prim & 0x40000000, 3 * 0x1000000 + (prim & 0xFFFFFF), 0x1000000 + prim)
    live = (prim != -1) & (tuv[:, 0] < 1e25)
    k = _i32(f[:, 14])
    assert np.array_equal(hit, live)
    assert np.array_equal(_i32(f[hit, 7]), code[hit])
    assert np.array_equal(_i32(rays[hit, 3]), _i32(tuv[hit, 0]))
    assert (rays[~hit, 3] == -1).all() and (k[~hit] == 0).all()
    assert (k > 0).sum() > 100000 and k.max() <= 4


def test_through_errors(pt, renderer_mod):
    wl = pt.scenes.build("C3", 96, 54)
    r = renderer_mod.Renderer(96, 54)
    r.load_workload(wl)
    L, h = r._L, r._h
    TR = renderer_mod.ThroughRule
    out = np.zeros((54, 96, 16), f32)
    n = C.c_int64(7)
    good = TR(4, 0.8, 1, 1)
    assert L.pt_read_features_through(h, None, out.ctypes.data) == -1
    assert L.pt_read_features_through(None, C.byref(good), out.ctypes.data) == -1
    assert L.pt_read_features_through(h, C.byref(good), None) == -1
    for bad in (TR(-1, 0.8, 1, 1), TR(9, 0.8, 1, 1), TR(4, 0.0, 1, 1), TR(4, -0.5, 1, 1), TR(4, 1.5, 1, 1), TR(4, float("nan"), 1, 1), TR(4, 0.8, 4, 1),
                TR(4, 0.8, -1, 1), TR(4, 0.8, 1, 2), TR(4, 0.8, 1, -1)):
        assert L.pt_read_features_through(h, C.byref(bad), out.ctypes.data) == -1
        assert L.pt_read_through_rays(h, C.byref(bad), out.ctypes.data) == -1
        assert L.pt_fill_frame_through(h, C.byref(bad), 0.3, 0.05, 0.1, 0.0, out.ctypes.data, C.byref(n)) == -1 and n.value == 0
        assert L.pt_denoise_guided_through(h, C.byref(bad), 5, 2.0, 0.3, 0.05, 0.1, 4, 0.0, out.ctypes.data) == -1
        assert L.pt_read_display_denoised_guided_through(h, C.byref(bad), 5, 2.0, 0.3, 0.05, 0.1, 4, 0.0, 1, out.ctypes.data) == -1
    for edge in (TR(0, 1.0, 0, 0), TR(8, 1e-6, 3, 1)):
        assert L.pt_read_features_through(h, C.byref(edge), out.ctypes.data) == 0
    # the errors of the calls of include/pt_fill.h
    assert L.pt_fill_frame_through(h, C.byref(good), 0.0, 0.05, 0.1, 0.0, out.ctypes.data, None) == -1
    assert L.pt_fill_frame_through(h, C.byref(good), 0.3, 0.05, 0.1, -1.0, out.ctypes.data, None) == -1
    assert L.pt_denoise_guided_through(h, C.byref(good), 5, 2.0, 0.3, 0.05, 0.1, 4, 0.0, out.ctypes.data) == -1      # no moments
    assert L.pt_fill_frame_through(h, C.byref(good), 0.3, 0.05, 0.1, 0.0, out.ctypes.data, None) == 0
    r.close()
    # PT_THROUGH_KEY packs the first-hit material into 12 bits: 4097 materials are refused with the key and served without it
    m = np.asarray(wl.buffers[14], f32).reshape(-1)
    me = int(m[0])
    many = np.zeros(me * 4097 + 1, f32)
    many[:m.size] = m
    for j in range((m.size - 1) // me, 4097):
        many[me * j + 1: me * j + me] = m[1:me]
    b = dict(wl.buffers); b[14] = many
    r = renderer_mod.Renderer(96, 54)
    r.load_workload(pt.scenes.Workload("C3_4097", 96, 54, b, wl.sky, wl.sample_res, wl.max_bounces, wl.info))
    assert r._L.pt_read_features_through(r._h, C.byref(good), out.ctypes.data) == -5
    assert r._L.pt_fill_frame_through(r._h, C.byref(good), 0.3, 0.05, 0.1, 0.0, out.ctypes.data, None) == -5
    assert r._L.pt_read_features_through(r._h, C.byref(TR(4, 0.8, 1, 0)), out.ctypes.data) == 0
    want = np.zeros_like(out)
    r.close()
    r = renderer_mod.Renderer(96, 54)
    r.load_workload(wl)
    assert r._L.pt_read_features_through(r._h, C.byref(TR(4, 0.8, 1, 0)), want.ctypes.data) == 0 and _bits_equal(out, want)
    r.close()
    part = renderer_mod.Renderer(96, 54, shard_rank=0, shard_count=2)
    part.load_workload(wl)
    assert part._L.pt_fill_frame_through(part._h, C.byref(good), 0.3, 0.05, 0.1, 0.0, out.ctypes.data, None) == -5
    part.close()
