"""GPU: the rows of csrc/hip/pt_image_args.hpp against the wrappers as compiled.  On one single-device context (C3 at 32 x 18: nothing here depends
on the size, and a refusal returns before any device work), through renderer.lib() and ctypes directly, so that no Python default stands between
the test and the library: for every entry point one refused call per refusal text of its row, code and pt_last_error() against the lines of
tests/golden/image_args_parent.json (the CPU test, tests/test_image_args.py, holds the stand-alone program to the same file); then one accepted call
with every field at a bound."""
import ctypes as C
import json

import numpy as np
import pytest

from test_image_args import BASE, GOLDEN, from_bits

pytestmark = pytest.mark.gpu

W, H = 32, 18
I64 = C.c_int64


def _parse(line):
    """a `call` line of the scripts -> (entry point, the pointers present, {field: value})"""
    words = line.split()
    assert words[0] == "call" and words[2].startswith("has=")
    values = {}
    for w in words[3:]:
        k, v = w.split("=", 1)
        values[k] = from_bits(int(v[2:], 16)) if v.startswith("f:") else int(v)
    return words[1], set(words[2][4:].split(",")) - {"-"}, values


def _call(L, mod, ctx, bufs, name, has, v):
    """the entry point through ctypes: pointers absent from `has` are NULL, every other argument is v's (BASE's where the row does not look)"""
    v = dict(BASE, **v)
    c = ctx if "ctx" in has else None
    buf = bufs["image"].ctypes.data if "buffer" in has else None
    seeds = bufs["seeds"].ctypes.data if "seeds" in has else None
    mask = bufs["mask"].ctypes.data if "mask" in has else None
    thru = C.byref(mod.ThroughRule(v["thru.max_depth"], v["thru.min_weight"], v["thru.lobes"], v["thru.flags"])) if "thru" in has else None
    guided = C.byref(mod.GuidedRule(v["guided.iterations"], v["guided.sigma_lum"], v["guided.sigma_normal"], v["guided.sigma_depth"], v["guided.sigma_albedo"],
                                    v["guided.min_frames"], v["guided.rel_err"], v["guided.abs_err"], v["guided.max_frames"])) if "rule" in has else None
    n, n2 = I64(-7), I64(-7)
    sig = (v["sigma0"], v["sigma1"], v["sigma2"], v["sigma3"])
    filt = (v["iterations"],) + sig
    rep = (v["max_history"], v["depth_tol"], v["normal_tol"], v["flags"])
    nf, floor, mf = v["n_frames"], v["albedo_floor"], v["min_frames"]
    f = getattr(L, name)
    if name in ("pt_motion_mark", "pt_history_hold"):
        return f(c)
    if name == "pt_record_moments":
        return f(c, 1)
    if name in ("pt_read_moments", "pt_write_moments", "pt_read_features"):
        return f(c, buf)
    if name == "pt_denoise":
        return f(c, *filt, buf)
    if name == "pt_read_display_denoised":
        return f(c, *filt, 0, buf)
    if name == "pt_denoise_guided":
        return f(c, *filt, mf, buf)
    if name == "pt_read_display_denoised_guided":
        return f(c, *filt, mf, 0, buf)
    if name in ("pt_denoise_guided_demod", "pt_denoise_guided_filled"):
        return f(c, *filt, mf, floor, buf)
    if name in ("pt_read_display_denoised_guided_demod", "pt_read_display_denoised_guided_filled"):
        return f(c, *filt, mf, floor, 0, buf)
    if name == "pt_reproject_frame":
        return f(c, *rep, C.byref(n))
    if name in ("pt_reproject_frame_demod", "pt_reproject_frame_moved"):
        return f(c, *rep, floor, C.byref(n))
    if name == "pt_reproject_frame_through":
        rule = C.byref(mod.ReprojectThroughRule(rep[0], rep[1], rep[2], v["point_tol"], v["radius"], rep[3])) if "rule" in has else None
        return f(c, thru, rule, C.byref(n), C.byref(n2))
    if name == "pt_reproject_frame_bilinear":
        rule = C.byref(mod.ReprojectBilinearRule(rep[0], rep[1], rep[2], v["snap"], floor, rep[3])) if "rule" in has else None
        return f(c, rule, C.byref(n), C.byref(n2))
    if name == "pt_history_merge":
        rule = C.byref(mod.ValidateRule(v["validate.radius"], v["validate.z_lo"], v["validate.z_hi"], v["validate.normal_tol"])) if "rule" in has else None
        return f(c, rule, None, C.byref(n))
    if name == "pt_render_mask":
        return f(c, 1, nf, seeds, mask, C.byref(n))
    if name == "pt_select_guided":
        return f(c, guided, buf, C.byref(n))
    if name == "pt_select_guided_demod":
        return f(c, guided, floor, buf, C.byref(n))
    if name == "pt_render_adaptive_guided":
        return f(c, 1, nf, seeds, guided, C.byref(n))
    if name == "pt_render_adaptive_guided_demod":
        return f(c, 1, nf, seeds, guided, floor, C.byref(n))
    if name == "pt_render_interleaved":
        return f(c, 1, nf, seeds, v["stride"], v["phase_x"], v["phase_y"], C.byref(n))
    if name == "pt_fill_frame":
        return f(c, *sig[1:], floor, buf, C.byref(n))
    if name in ("pt_read_features_through", "pt_read_through_rays"):
        return f(c, thru, buf)
    if name == "pt_fill_frame_through":
        return f(c, thru, *sig[1:], floor, buf, C.byref(n))
    if name == "pt_denoise_guided_through":
        return f(c, thru, *filt, mf, floor, buf)
    if name == "pt_read_display_denoised_guided_through":
        return f(c, thru, *filt, mf, floor, 0, buf)
    assert name == "pt_render_adaptive", name
    return f(c, 1, nf, seeds, v["rel_err"], v["abs_err"], mf, v["max_frames"], C.byref(n))


def test_the_wrappers_answer_as_their_rows_do(pt, renderer_mod):
    want = json.load(open(GOLDEN))
    L = renderer_mod.lib()
    wl = pt.scenes.build("C3", W, H)
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl)
    r.record_moments()
    r.render_batch(1, [pt.scenes.frame_seed(k) for k in range(1, 5)])
    bufs = dict(image=np.zeros(W * H * 16, np.float32), seeds=np.array([pt.scenes.frame_seed(5)], np.int32), mask=np.zeros(W * H, np.uint8))
    assert len(want["one"]) == 33
    replayed = set()
    for name, items in want["one"].items():
        pointers = [item for item in items if item not in BASE]
        seen = set()
        for item, answers in items.items():
            for value, (code, m) in answers.items():
                if code == 0 or m in seen:
                    continue
                seen.add(m)                                           # the first script of the file that this text answers
                has = set(pointers) - {item}
                v = {} if item in pointers else {item: int(value) if isinstance(BASE[item], int) else from_bits(int(value, 16))}
                rc = _call(L, renderer_mod, r._h, bufs, name, has, v)
                assert (rc, L.pt_last_error().decode()) == (code, want["messages"][m]), (name, item, value)
                replayed.add(m)
    assert replayed == set(range(1, len(want["messages"]))) and want["messages"][0] == ""      # every message of the file
    # every field at a bound: accepted, and the device work behind it runs
    for name, (line, answer) in want["at_bounds"].items():
        assert answer == "rc=0 msg="
        entry, has, v = _parse(line)
        assert entry == name
        rc = _call(L, renderer_mod, r._h, bufs, name, has, v)
        assert rc == 0, (name, rc, L.pt_last_error().decode())
    r.close()
