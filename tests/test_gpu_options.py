"""GPU: pt_set_option on a live Renderer (C3 at 32 x 18: nothing here depends on the size).  The CPU test runs the option table
(csrc/hip/pt_options.hpp) alone; this ties it to the call around it, to the two queries the context answers, and to the scene rebuild the table asks for.

  * the "replay" script of tests/test_options.py — every option with a value that is not its default, a refused value and its default again, three
    numbers that are no option — call by call against the codes and messages tests/golden/options_parent.json holds; the queries 12 and 13 before
    and after a render, and a null context;
  * options that change the scene's layout, set on a context that has already rendered, rebuild the scene: the same two frames then give the same
    bits as under the defaults (the exact numeric contract makes every layout and every intersect kernel give the same image; a stale layout under
    the new options would not)."""
import json

import numpy as np
import pytest

from test_options import GOLDEN, QUERIES, REPLAY, fields

pytestmark = pytest.mark.gpu

W, H = 32, 18
PT_ERR_ARG, PT_ERR_UNSUPPORTED = -1, -5


def _set(renderer_mod, r, option, value, handle=True):
    """pt_set_option by number -> (code, message)"""
    try:
        renderer_mod._check(r._L.pt_set_option(r._h if handle else None, int(option), int(value)))
        return 0, ""
    except renderer_mod.PtError as e:
        return e.code, str(e).split("] ", 1)[1]


def test_a_live_context_answers_as_the_table_does(pt, renderer_mod):
    want = json.load(open(GOLDEN))["sequences"]["replay"]
    assert len(want) == len(REPLAY) >= 40
    wl = pt.scenes.build("C3", W, H)
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl)
    assert _set(renderer_mod, r, 0, 0, handle=False) == (PT_ERR_ARG, "null context")
    asked = set()
    for line, answer in zip(REPLAY, want):
        _, option, value = line.split()
        rc, query, _, _, msg = fields(answer)
        got = _set(renderer_mod, r, option, value)
        if query:                                                     # before any render: C3 runs on the hand-written kernel, which has not been launched yet
            assert int(option) in QUERIES
            assert got == ((0, "") if int(option) == 12 else (PT_ERR_UNSUPPORTED, "the hand-written intersect kernel has been launched 0 times")), line
        else:
            assert got == (rc, msg), line
        asked.add(int(option))
    assert asked == set(range(22)) | {-1, 22}                         # every option, 15 and two more numbers that are none
    # every option is at its default again: the render runs as a fresh context's would
    r.reset_frame()
    r.render_batch(1, [pt.scenes.frame_seed(1)])
    assert _set(renderer_mod, r, 12, 0) == (0, "")
    assert _set(renderer_mod, r, 13, 0) == (0, "")
    code, msg = _set(renderer_mod, r, 13, 1 << 40)
    assert code == PT_ERR_UNSUPPORTED and msg.startswith("the hand-written intersect kernel has been launched ") and int(msg.split()[-2]) >= 1
    assert _set(renderer_mod, r, 12, 1 << 40) == (0, "")              # (12 does not read its value)
    r.close()


def test_layout_options_set_after_a_render_rebuild_the_scene(pt, renderer_mod):
    wl = pt.scenes.build("C3", W, H)
    seeds = [pt.scenes.frame_seed(f) for f in (1, 2)]
    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl)
    r.reset_frame()
    r.render_batch(1, seeds)
    a = r.read_frame().copy()
    assert a.shape == (H, W, 4) and np.isfinite(a).all() and float(a[..., :3].max()) > 0.0
    # the context has rendered: its scene is built and clean.  Each of the layout options marks it for a rebuild; the intersect kernel as the default
    # chooses it (the hand-written one), then the compiled persistent one, then the simple one
    for extend_mode in (2, 1, 0):
        for name, value in (("lds_budget", 4096), ("bfs_nodes", 64), ("stack_mode", 2), ("asm_node_layout", 1), ("index_stack_8bit", 1), ("extend_cache_bytes", 2048)):
            r.set_option(name, value)
        r.set_option("extend_mode", extend_mode)
        r.reset_frame()
        r.render_batch(1, seeds)
        assert np.array_equal(a.view(np.uint32), r.read_frame().view(np.uint32)), extend_mode
    r.close()
