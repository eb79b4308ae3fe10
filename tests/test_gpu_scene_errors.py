"""GPU: a scene the layout step refuses (tests/test_scene_layout.py) is refused through the real ABI with the same code and text, before anything
is uploaded, and the context renders the valid scene afterwards exactly as a fresh context does."""
import numpy as np
import pytest

from conftest import frames_equal
from test_scene_layout import E_CHILD, E_ELLIPLEN, E_TRIMAT, E_TWICE, one_ellipsoid

pytestmark = pytest.mark.gpu
W, H, FRAMES = 48, 27, 2


@pytest.fixture(scope="module")
def t1(pt):
    return pt.scenes.build("T1", W, H)


def render(pt, r):
    r.reset_frame()
    for f in range(1, FRAMES + 1):
        r.render(f, pt.scenes.frame_seed(f))
    return r.read_frame()


@pytest.fixture(scope="module")
def valid_image(pt, renderer_mod, t1):
    r = renderer_mod.Renderer(W, H)
    r.load_workload(t1)
    img = render(pt, r)
    r.close()
    return img


def broken(wl, which):
    """(binding, contents) of one buffer of T1 made inconsistent"""
    tree, tris = wl.buffers[11].copy(), wl.buffers[3].copy()
    if which == "child":
        tree[1] = tree.size // 3                                 # the root's left child: one past the last node
        return 11, tree, E_CHILD
    if which == "twice":
        tree[1] = 0                                              # ... the root itself
        return 11, tree, E_TWICE
    if which == "trimat":
        tris[36] = 1000.0
        return 3, tris, E_TRIMAT
    return 7, one_ellipsoid(0.0)[:11], E_ELLIPLEN               # a count of one over ten floats


def refuse(pt, renderer_mod, r, wl, which):
    binding, contents, text = broken(wl, which)
    r.set_buffer(binding, contents)
    with pytest.raises(renderer_mod.PtError) as e:
        r.render(1, pt.scenes.frame_seed(1))
    assert e.value.code == -4 and str(e.value) == f"[-4] {text}"
    r.set_buffer(binding, wl.buffers[binding])


@pytest.mark.parametrize("which", ["child", "twice", "trimat", "ellip"])
def test_refused_scene_then_the_valid_one(pt, renderer_mod, t1, valid_image, which):
    assert int(t1.buffers[13][1]) == 0 and tuple(t1.buffers[11][1:3]) != (-1, -1)      # object 0's root is node 0, an inner node
    r = renderer_mod.Renderer(W, H)
    r.load_workload(t1)
    refuse(pt, renderer_mod, r, t1, which)
    got = render(pt, r)
    r.close()
    assert frames_equal(got, valid_image)


def test_valid_scene_refused_scene_valid_scene(pt, renderer_mod, t1, valid_image):
    r = renderer_mod.Renderer(W, H)
    r.load_workload(t1)
    assert frames_equal(render(pt, r), valid_image)
    for which in ("child", "twice", "trimat", "ellip"):
        refuse(pt, renderer_mod, r, t1, which)
    got = render(pt, r)
    r.close()
    assert frames_equal(got, valid_image)
    assert np.isfinite(got[..., 3]).all() and (got[..., 3] > 0).any()
