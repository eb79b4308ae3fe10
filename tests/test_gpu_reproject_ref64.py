"""GPU: k_reproject (csrc/hip/pt_reproject.hip) against the float64 scene-space reference of tests/_reproject_ref64.py, through the four calls
that share its text — pt_reproject_frame (pt_reproject_frame_demod), pt_reproject_frame_bilinear, pt_motion_mark + pt_reproject_frame_moved and
pt_reproject_frame_moved_bilinear — each with albedo_floor 0 and > 0, so that all eight instantiations run, on the cases of
tests/_reproject_cases.py and the probe images of the reference (FRAME and T name their own pixels).

Every other GPU test of these calls holds the kernel to a float32 twin that restates the same header lines on the same feature records; here
the expectation comes from the scene and the two cameras alone.  With normal_tol = -1 material and depth decide, and the reference knows both:
on a decided pixel the kernel's keep / reject and its source must be the reference's, the blended mean and count within BOUND_K units
(tests/_reproject_cases.py: four times what tests/test_reproject_ref64.py measures for the twins; the kernel equals them bit for bit, so it adds
nothing of its own).  The scenes are untextured, so the carried albedo ratio of a same-material pair is exactly 1 and the demodulated calls
have the plain calls' expectation.  Undecided pixels are not asserted here: the twin tests hold them bit for bit.  Every reference is computed
once per process."""
import numpy as np
import pytest

import _reproject_cases as RC
import _reproject_ref64 as RR

pytestmark = pytest.mark.gpu

GEOMETRY = (3, 7, 10, 11, 12, 13)
FLOORS = (0.0, 0.2)


def _setcam(r, cam):
    r.set_buffer(0, np.asarray(cam[0], np.float32))
    r.set_buffer(1, np.asarray(cam[1], np.float32))


class Device:
    """one context per case: every call starts from the probe images under camera A in the scene `then`"""

    def __init__(self, renderer_mod, case):
        self.c = case
        self.r = renderer_mod.Renderer(case.W, case.H)
        self.r.load_workload(case.then)
        self.r.record_moments(True)
        self.fr, self.T = RR.probe_images(case.W, case.H)

    def run(self, rule, cap, floor, normal_tol=-1.0):
        """(FRAME, T, n_kept, n_blended or None)"""
        r, c = self.r, self.c
        if c.moved:
            for b in GEOMETRY:
                r.set_buffer(b, c.then.buffers[b])
        _setcam(r, c.A)
        r.set_buffer(2, RC.NO_MOUSE)
        r.write_frame(self.fr)
        r.write_moments(self.T)
        if c.moved:
            r.motion_mark()
            for b in GEOMETRY:
                r.set_buffer(b, c.now.buffers[b])
        _setcam(r, c.B)
        blended = None
        if rule == "nearest":
            if c.moved:
                kept = r.reproject_frame_moved(cap, RC.DEPTH_TOL, normal_tol, c.allm, floor)
            else:
                kept = r.reproject_frame(cap, RC.DEPTH_TOL, normal_tol, c.allm, floor if floor else None)
        else:
            call = r.reproject_frame_moved_bilinear if c.moved else r.reproject_frame_bilinear
            kept, blended = call(cap, RC.DEPTH_TOL, normal_tol, rule, c.allm, floor)
        return r.read_frame(), r.read_moments(), kept, blended

    def close(self):
        self.r.close()


def _off_centre(out):
    """the kept pixels whose mean is not an old pixel's centre: blended from two or more of the probe image's pixels"""
    with np.errstate(all="ignore"):
        mx, my = out[..., 0] / out[..., 3], out[..., 1] / out[..., 3]
    return (out[..., 3] > 0) & ((mx - np.floor(mx) != 0.5) | (my - np.floor(my) != 0.5))


@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("name", RC.NAMES)
def test_the_kernel_agrees_with_the_reference(pt, renderer_mod, name, floor):
    c = RC.case(pt, name)
    dev = Device(renderer_mod, c)
    n_pix = c.W * c.H
    loose, counts = {}, {}
    for rule in ("nearest",) + RC.SNAPS:
        e = RC.expect(pt, name, rule)
        for cap in (64.0, 4.0):
            out, T, kept, blended = dev.run(rule, cap, floor)
            f = RR.compare(e, out, T, cap)
            tag = (name, floor, rule, cap)
            print(f"{tag}: decided {f.n_decided} of {n_pix}, kept {f.n_kept} of them; device kept {kept}, blended {blended}; K {f.k:.2f} at {f.where}")
            assert f.wrong_decision == 0 and f.wrong_source == 0, (tag, f.wrong_decision, f.wrong_source)
            assert f.k <= RC.BOUND_K, (tag, f.k, f.where)
            assert kept == int((out[..., 3] > 0).sum()), tag
            assert np.array_equal(T[..., 2] > 0, out[..., 3] > 0), tag              # every probe pixel has moments: T is kept where FRAME is
            if rule != "nearest":
                seen = int(_off_centre(out).sum())
                if cap != 64.0:                                                     # the cap rescales a copied pixel, and changes no tap
                    assert blended == counts[rule] and kept == int((loose[(rule, 64.0)][..., 3] > 0).sum()), (tag, blended, counts[rule])
                elif rule > 0:
                    assert blended == seen, (tag, blended, seen)
                else:                   # a tap of weight 2^-20 moves no float32 mean: without snapping the count read off the output is a lower bound
                    assert seen <= blended <= kept, (tag, blended, seen)
                counts.setdefault(rule, blended)
            elif cap == 64.0:
                assert not _off_centre(out).any(), tag                              # below the cap the nearest rule copies: every mean is a centre
            loose[(rule, cap)] = out
    # the normal test only takes away: the kept set shrinks, and what the nearest rule still keeps it keeps from the same source
    for rule in ("nearest", RC.SNAPS[0]):
        out, T, kept, _ = dev.run(rule, 64.0, floor, normal_tol=0.9)
        k9, k1 = out[..., 3] > 0, loose[(rule, 64.0)][..., 3] > 0
        assert not (k9 & ~k1).any() and kept == int(k9.sum()), (name, floor, rule)
        if rule == "nearest":
            assert np.array_equal(out[k9].view(np.uint32), loose[(rule, 64.0)][k9].view(np.uint32)), (name, floor)
    dev.close()


def test_every_instantiation_kept_and_rejected_something(pt, renderer_mod):
    """the calls above are not vacuous: on M1 under a moving camera each of the eight keeps and rejects decided pixels, and the bilinear ones
    blend"""
    for name in ("C2", "M1cam"):
        c = RC.case(pt, name)
        dev = Device(renderer_mod, c)
        for floor in FLOORS:
            for rule in ("nearest", RC.SNAPS[0]):
                e = RC.expect(pt, name, rule)
                out, _, kept, blended = dev.run(rule, 64.0, floor)
                got = out[..., 3] > 0
                assert (e.decided & e.kept & got).sum() > 0.5 * c.W * c.H and (e.decided & ~e.kept & ~got).sum() > 20, (name, floor, rule)
                if rule != "nearest":
                    assert blended > 0.5 * c.W * c.H and (e.decided & (e.taps == 4)).sum() > 0.25 * c.W * c.H, (name, floor, rule)
        dev.close()
