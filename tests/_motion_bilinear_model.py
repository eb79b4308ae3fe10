"""float32 model of the reprojection across moved geometry with bilinear taps of include/pt_motion_bilinear.h: the composition of the two models it
is built from, so that tests/test_gpu_motion_bilinear.py can hold the device to it bit for bit (not a test module).

tests/_motion_model.py's mapped records put P' in D and N~ in N with t = 1 under a current origin of (-0, -0, -0), and leave F1 (the hit code, Kd)
and F2's material word alone; a hit the motion rule rejects gets t = NaN.  Handed to tests/_reproject_bilinear_model.py, its own step 2 reproduces
P' and tests N~, and steps 3-9, the overlay (fin's mouse) and the carried albedo are that model's own, bit for bit."""
from _motion_model import mapped_records
from _reproject_bilinear_model import reproject_bilinear


def reproject_moved_bilinear(rn, rh, frame, T, fin_h, fin_n, mat_vd, rot_h, tri_now, tri_then, el_now, el_then, max_history, depth_tol, normal_tol,
                             snap=1.0 / 64, all_materials=False, floor=0.0, detail=False):
    """The new FRAME, the new T (None when T is None), the kept and the blended count of pt_reproject_frame_moved_bilinear (and the detail dict of
    reproject_bilinear).  rn, rh, tri_*, el_*: as _motion_model.reproject_moved; the rest as _reproject_bilinear_model.reproject_bilinear."""
    r, fin = mapped_records(rn, fin_n, tri_now, tri_then, el_now, el_then)
    return reproject_bilinear(r, rh, frame, T, fin_h, fin, mat_vd, rot_h, max_history, depth_tol, normal_tol, snap, all_materials, floor, detail)
