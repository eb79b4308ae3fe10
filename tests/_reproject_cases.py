"""The cases tests/test_reproject_ref64.py (CPU, the float32 twins) and tests/test_gpu_reproject_ref64.py (GPU, k_reproject) share: a scene as
it was under the image's camera A, the scene as it is under the current camera B, and the float64 reference of tests/_reproject_ref64.py for
the pair, computed once per process (not a test module).  The mouse is off-screen throughout: the overlay stays with the twins.

Sizes: 96 x 54 (one full and one half block column, three block rows and a part), 100 x 7 (every block partial), 65 x 17 (one lane and one row
into the next block).  A is the scene's own rotation or (0.15, -0.4, 0.3), the only path through RZ.  B: the small forward / strafe / yaw of
tests/test_gpu_reproject.py, pitch and roll changed by 0.05, a dolly of 0.8 that halves the distance to the room's middle (many new pixels per
old one), a yaw by 2.0 that leaves part of the view behind A or off its image."""
import copy

import numpy as np

import _intersect_cases as IC
import _reproject_ref64 as RR
from test_gpu_reproject import move

f32 = np.float32
NO_MOUSE = np.array([-1.0e6, -1.0e6, 0.0], f32)
DEPTH_TOL = 0.02
SNAPS = (1.0 / 64, 0.0)
SMALL = dict(forward=0.03, strafe=0.02, yaw=0.02)
ROLLED = (0.15, -0.4, 0.3)

STATIC = {
    "C2": dict(scene="C2", mv=SMALL),
    "C3": dict(scene="C3", mv=SMALL),
    "C3all": dict(scene="C3", mv=SMALL, allm=True),
    "C1": dict(scene="C1", mv=SMALL),
    "C6": dict(scene="C6", size=(65, 17), kw=dict(groups=64, nu=8, nv=8), mv=SMALL),      # 8192 triangles: the small image keeps the brute force short
    "C2roll": dict(scene="C2", size=(65, 17), rot=ROLLED, drot=(0.05, 0.0, 0.05)),
    "C2dolly": dict(scene="C2", size=(100, 7), mv=dict(forward=0.8)),
    "C2yaw2": dict(scene="C2", size=(65, 17), rot=ROLLED, mv=dict(yaw=2.0)),
}
MOVED = {
    "M1": dict(kind="m1"),                                           # 0 -> 3: a rigid move of box, sphere and poster, the ellipsoid moved and grown
    "M1cam": dict(kind="m1", mv=SMALL),
    "M5": dict(kind="m5", mv=SMALL),                                 # rest -> step 3: morphed, skinned, re-smoothed: no rigid part
    "M1ell": dict(kind="ell", stretch=(1.5, 0.8, 1.2), r=0.25, centre=(0.03, 0.27, -0.43)),
    "M1ellrot": dict(kind="ell", stretch=(1.5, 0.8, 1.2), r=0.25, centre=(0.03, 0.27, -0.43), rot=(0.0, 0.3, 0.0)),
}
# |mean - ref| and |a - ref| / 7 <= BOUND_K units of tests/_reproject_ref64.compare: four times the largest multiple measured for the twins over
# every case, rule and cap of tests/test_reproject_ref64.py (MEASURED_K there)
MEASURED_K = 47.56
BOUND_K = 4.0 * MEASURED_K
SAME_VIEWS = {"C3all": "C3"}                                        # the same scene and cameras under another flag
NAMES = list(STATIC) + list(MOVED)


class Case:
    """then, now: workloads (every binding) of the scene under A and under B; moved: geometry differs; allm: PT_REPROJECT_ALL_MATERIALS"""

    def __init__(self, name, then, now, moved, allm):
        self.name, self.then, self.now, self.moved, self.allm = name, then, now, moved, allm
        self.W, self.H = then.W, then.H
        self.A = (then.buffers[0], then.buffers[1])
        self.B = (now.buffers[0], now.buffers[1])


def _with(wl, **bind):
    out = copy.copy(wl)
    out.buffers = dict(wl.buffers)
    for k, v in bind.items():
        out.buffers[int(k[1:])] = v
    out.buffers[2] = NO_MOUSE
    return out


def _camera_b(A, spec):
    org, rot = move(*A, **spec.get("mv", {}))
    return org, (rot + np.asarray(spec.get("drot", (0, 0, 0)), f32)).astype(f32)


def _ellipsoid(b7, stretch, r, centre, rot=(0.0, 0.0, 0.0)):
    e = np.array(b7, f32)
    assert int(e[0]) == 1
    e[1:4], e[4:7], e[7:10], e[10] = centre, stretch, rot, r
    return e


def case(pt, name):
    def make():
        S = pt.scenes
        if name in STATIC:
            spec = STATIC[name]
            w, h = spec.get("size", (96, 54))
            wl = S.build(spec["scene"], w, h, **spec.get("kw", {}))
            rot = np.asarray(spec.get("rot", wl.buffers[1]), f32)
            then = _with(wl, b1=rot)
            org, rot_b = _camera_b((then.buffers[0], rot), spec)
            return Case(name, then, _with(then, b0=org, b1=rot_b), False, spec.get("allm", False))
        spec = MOVED[name]
        if spec["kind"] == "m1":
            then, now = _with(S.m1_moving(0, textured=False)), S.m1_moving(3, textured=False)
        elif spec["kind"] == "m5":
            old, new = IC.m5(pt, 3)
            then = _with(S.m5_rippling(3)[0])
            assert np.array_equal(then.buffers[3], old.buffers[3])
            now = _with(then, b3=new.buffers[3], b10=new.buffers[10])
        else:
            then = _with(S.m1_moving(0, textured=False))
            now = _with(then, b7=_ellipsoid(then.buffers[7], spec["stretch"], spec["r"], spec["centre"], spec.get("rot", (0.0, 0.0, 0.0))))
        org, rot_b = _camera_b((then.buffers[0], then.buffers[1]), spec)
        return Case(name, then, _with(now, b0=org, b1=rot_b), True, False)
    return IC._once(("reproject case", name), make)


def scene(buffers):
    """{3, 7} for the reference: the triangles no leaf names collapsed (tests/_intersect_cases.in_scene), binding 7 as it is"""
    return {3: IC.in_scene(buffers)[3], 7: buffers[7]}


def reference(pt, name):
    def make():
        c = case(pt, name)
        now = scene(c.now.buffers)
        then = scene(c.then.buffers) if c.moved else now
        views = None
        if name in SAME_VIEWS:
            base = reference(pt, SAME_VIEWS[name])
            views = (base.new, base.old)
        return RR.Reference(now, then, c.now.buffers[14], RR.Camera.of(c.then.buffers), RR.Camera.of(c.now.buffers), c.W, c.H, DEPTH_TOL, c.allm, views)
    return IC._once(("reproject reference", name), make)


def expect(pt, name, rule):
    """the Expect of a rule: "nearest", or a snap"""
    def make():
        ref = reference(pt, name)
        return ref.nearest() if rule == "nearest" else ref.bilinear(rule)
    return IC._once(("reproject expect", name, rule), make)
