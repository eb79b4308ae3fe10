"""GPU: the feature-record caches of a context (first-hit and seen-through records, each under the current inputs and under the image's
camera) never serve a stale record.  No model: a sequence of calls runs on one warm context, and after each call FRAME, T and the returned
counts are compared bit for bit with the same call on a cold context: a fresh one, given the previous result by pt_write_frame +
pt_write_moments under the previous camera, then moved to the new inputs."""
import numpy as np
import pytest

from test_gpu_motion import GEOMETRY
from test_gpu_reproject import _setcam, move
from test_gpu_reproject_through import CHAINS, SMALL, _inject

pytestmark = pytest.mark.gpu

W, H = 96, 54
SHALLOW = dict(max_depth=2, min_weight=0.9, lobes=1, key=True)    # shorter chains than CHAINS, reflections only: other records


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _cams(wl):
    A = (wl.buffers[0], wl.buffers[1])
    B = move(*A, **SMALL)
    return A, B, move(*B, **SMALL)


def _result(r, counts):
    return counts, r.read_frame(), r.read_moments()


def _through(r):
    return r.reproject_frame_through(r.through_rule(**CHAINS), r.reproject_through_rule())


# ---- C3: every call as (name, the camera of the image before it, a new image or None, what only the warm context does before the call, the
# call under comparison).  The prelude leaves FRAME and T alone and is what would make a stale record: the cold context never runs it.
def _c3_calls(wl):
    A, B, Cc = _cams(wl)
    fr2, T2 = _inject(W, H, seed=11)

    def shallow(r):
        deep = r.read_features_through(r.through_rule(**CHAINS))
        # the seen-through records under another rule, no upload after it; served under the default chains they would be the wrong ones (the
        # float32 model of tests/_through_model.py: 464 of the 645 chain pixels differ at this camera)
        assert not _same(r.read_features_through(r.through_rule(**SHALLOW)), deep)

    return [("through A->B", A, None, None, lambda r: (_setcam(r, *B), _through(r))[1]),
            ("again, nothing uploaded", B, None, None, _through),
            ("another rule, then the default chains", B, None, shallow, lambda r: r.reproject_frame_through()),
            ("first hit B->C", B, None, None, lambda r: (_setcam(r, *Cc), r.reproject_frame())[1]),
            ("next image written under C, back to A", Cc, (fr2, T2), None, lambda r: (_setcam(r, *A), r.reproject_frame())[1])]


def _cold_c3(pt, renderer_mod):
    """the chain of cold results: call k on a fresh context that was given result k-1"""
    wl = pt.scenes.build("C3", W, H)
    image = _inject(W, H)
    out = []
    for name, cam, fresh, _, call in _c3_calls(wl):
        image = fresh or image
        r = renderer_mod.Renderer(W, H)
        r.load_workload(wl)
        _setcam(r, *cam)
        r.write_frame(image[0])
        r.write_moments(image[1])
        res = _result(r, call(r))
        r.close()
        out.append(res)
        image = res[1:]
    return out


@pytest.fixture(scope="module")
def cold_c3(pt, renderer_mod):
    return _cold_c3(pt, renderer_mod)


@pytest.mark.parametrize("kw", [dict(device=0), dict(devices=[0, 0])], ids=["one stream", "two streams"])
def test_c3_warm_context_equals_cold_contexts(pt, renderer_mod, cold_c3, kw):
    wl = pt.scenes.build("C3", W, H)
    r = renderer_mod.Renderer(W, H, **kw)
    r.load_workload(wl)
    fr, T = _inject(W, H)
    r.write_frame(fr)
    r.write_moments(T)
    for k, ((name, cam, fresh, prelude, call), want) in enumerate(zip(_c3_calls(wl), cold_c3)):
        if fresh:                                               # the image changes without an upload
            r.next_image()
            r.write_frame(fresh[0])
            r.write_moments(fresh[1])
        if prelude:
            prelude(r)
        got = _result(r, call(r))
        kept = got[0][0] if isinstance(got[0], tuple) else got[0]
        print(f"C3 {kw} step {k + 1} ({name}): counts {got[0]}, cold {want[0]}")
        assert got[0] == want[0], (name, got[0], want[0])
        assert _same(got[1], want[1]), (name, "FRAME")
        assert _same(got[2], want[2]), (name, "T")
        assert 0 < kept < W * H, (name, kept)
        if k == 0:
            assert got[0][1] > 300, got[0]                       # chain pixels: the comparison does not pass on an empty search
    r.close()


# ---- M1, steps 0 -> 4: the mark takes its records from the cache pt_reproject_frame filled, and the geometry upload drops all of them
def _upload(r, wl):
    for b in GEOMETRY:
        r.set_buffer(b, wl.buffers[b])


def test_m1_warm_context_equals_cold_contexts(pt, renderer_mod):
    wl0, wl4 = pt.scenes.m1_moving(0, W, H), pt.scenes.m1_moving(4, W, H)
    A, B, Cc = _cams(wl0)
    fr, T = _inject(W, H)

    def cold(image, cam, moved_scene, call):
        r = renderer_mod.Renderer(W, H)
        r.load_workload(wl0)
        if moved_scene:
            _upload(r, wl4)
        _setcam(r, *cam)
        r.write_frame(image[0])
        r.write_moments(image[1])
        res = _result(r, call(r))
        r.close()
        return res

    def moved(r):
        r.motion_mark()
        _upload(r, wl4)
        return r.reproject_frame_moved()

    r = renderer_mod.Renderer(W, H)
    r.load_workload(wl0)
    r.write_frame(fr)
    r.write_moments(T)
    steps = [("first hit A->B", A, False, lambda q: (_setcam(q, *B), q.reproject_frame())[1]),
             ("mark with nothing uploaded, geometry of step 4, moved", B, False, moved),
             ("first hit B->C in the moved scene", B, True, lambda q: (_setcam(q, *Cc), q.reproject_frame())[1])]
    image = (fr, T)
    for name, cam, moved_scene, call in steps:
        got = _result(r, call(r))
        want = cold(image, cam, moved_scene, call)
        print(f"M1 ({name}): kept {got[0]}, cold {want[0]}")
        assert got[0] == want[0], (name, got[0], want[0])
        assert _same(got[1], want[1]), (name, "FRAME")
        assert _same(got[2], want[2]), (name, "T")
        assert 0 < got[0] < W * H, (name, got[0])
        image = want[1:]
    r.close()
