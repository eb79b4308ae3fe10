"""GPU: six of the named scripts of tests/test_image_history.py replayed on a live Renderer (C3 at 32 x 18: nothing here depends on the size), each
call's code and message against the lines tests/golden/image_history_parent.json holds for that script.  The CPU test runs the image history
(csrc/hip/pt_image_history.hpp) under a stand-in for the context; this ties the stand-in to the calls pt_hip.hip and pt_image.hpp make around it."""
import json

import pytest

from test_image_history import GOLDEN, GPU_REPLAYED, NAMED

pytestmark = pytest.mark.gpu

W, H = 32, 18


def _call(r, wl, seed, line):
    verb = line.split()[0]
    if line == "inputs 1":
        return                                                       # the workload's camera, bound with it
    if verb == "render":
        r.render_batch(1, [seed])
    elif line == "upload materials ok":
        r.set_buffer(14, wl.buffers[14])
    elif line == "upload geometry ok":
        r.set_buffer(3, wl.buffers[3])
    elif line == "reproject through":
        r.reproject_frame_through()
    else:
        {"mark": r.motion_mark, "moved": r.reproject_frame_moved, "hold": r.history_hold, "merge": r.history_merge, "next-image": r.next_image,
         "reset": r.reset_frame, "reproject plain": r.reproject_frame, "reproject bilinear": r.reproject_frame_bilinear}[line]()


def test_a_live_context_answers_as_the_stand_in_does(pt, renderer_mod):
    want = json.load(open(GOLDEN))["traces"]
    wl = pt.scenes.build("C3", W, H)
    assert len(GPU_REPLAYED) == 6
    for name in GPU_REPLAYED:
        script = NAMED[name]
        answers = [line for line in want[name] if line.startswith("rc=")]
        assert script[0] == f"create {W} {H}" and len(answers) == len(script) - 1, name
        r = renderer_mod.Renderer(W, H)
        r.load_workload(wl)
        r.record_moments()                                            # (a hold asks for T before it asks the history)
        for line, answer in zip(script[1:], answers):
            code, msg = int(answer.split()[0][3:]), answer.split(" error=", 1)[1] if " error=" in answer else ""
            try:
                _call(r, wl, pt.scenes.frame_seed(1), line)
                got = (0, "")
            except renderer_mod.PtError as e:
                got = (e.code, str(e).split("] ", 1)[1])
            assert got == (code, msg), (name, line)
        r.close()
