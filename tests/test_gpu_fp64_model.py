"""The device's tracker and BA systems against the fp64 model (tests/fp64_model.py) on the photometric cases.

Metric as in tests/test_fp64_model.py: d = max |X - X64| / A over entries with A > 0.  The bar is not fixed:

    bar = min(max(4 d_oracle, 4 sqrt(n) 2^-24), 1e-3)

d_oracle is the CPU oracle's d on the same case, computed in the same test; n is the number of summed terms.  The
device sums in wave trees and block partials where the oracle sums sequentially: both are fp32 random walks about the
same fp64 value (the per-term arithmetic is pinned bit-equal elsewhere), hence the factor 4; the floor is the
random-walk size of n roundings, for cases where the oracle happens to land within an ulp.  Each test prints d_oracle,
d_device and the bar.

BA windows run under both linearize kernels: HS_LIN8=0 (hs_k_lin) and HS_LIN8=1 (hs_k_lin8).
"""
import os

import numpy as np
import pytest

import fp64_model as fm
import photo_cases as pc
from test_fp64_model import BA_SYSTEMS, CAP, ba_d, ba_oracle_systems, track_case, track_poses, tracker_d, tracker_model

pytestmark = pytest.mark.gpu


def bar(d_oracle, n):
    return min(max(4 * d_oracle, 4 * np.sqrt(n) * 2.0 ** -24), CAP)


def ba_window(scene, lin8, params=None):
    from hslam_amd.ba import BAWindow
    os.environ["HS_LIN8"] = "1" if lin8 else "0"
    try:
        return BAWindow(scene, params=params)
    finally:
        os.environ.pop("HS_LIN8", None)


def device_ba_case(n_frames, n_points, kind, lin8):
    """(scene, calib value, params, device window linearized once at that state, kernel name, that linearization's
    energy).  'calib': the device's own state after one GN step under the weak calibration prior (the C-ABI has no
    calibration setter), handed to the oracle and the model through the returned scene and calib value."""
    from hslam_amd._lib import default_params
    s = pc.make_photo_ba(n_frames, n_points, kind)
    cv, params = None, None
    if kind == "calib":
        params = pc.calib_params(default_params())
    g = ba_window(s, lin8, params)
    energy = g.linearizeAll(reset=True)
    if kind == "calib":
        s, cv = pc.stepped(s, g)
        energy = g.linearizeAll(reset=True)
    kernel = g.partition()["kernel"]
    assert kernel == ("hs_k_lin8" if lin8 else "hs_k_lin")
    return s, cv, params, g, kernel, energy


@pytest.mark.parametrize("name", list(pc.TRACK_CASES))
def test_tracker_device_against_model(name):
    from hslam_amd.track import CoarseTracker
    s, aff, o = track_case(name)
    g = CoarseTracker(s.width, s.height, s.K4, s.n_levels)
    g.set_scene(s)
    for which, T7 in track_poses(s).items():
        for lvl in range(s.n_levels):
            cut = g.params.coarseCutoffTH
            _, Hg, bg, ng = g.calcRes(lvl, T7, aff, cut)
            _, Ho, bo, no = o.calc_res(lvl, T7, aff, cut)
            H, b, A_H, A_b, n = tracker_model(s, o, lvl, T7, aff, o.params)
            assert ng == no == (n + 3) // 4 * 4
            for what, dg, do in zip("Hb", tracker_d(Hg, bg, H, b, A_H, A_b), tracker_d(Ho, bo, H, b, A_H, A_b)):
                br = bar(do, n)
                print(f"{name} {which} level {lvl} {what}: n {n}  d_oracle {do:.2e}  d_device {dg:.2e}  bar {br:.2e}")
                assert do <= CAP and dg <= br, (which, lvl, what, do, dg, br)
    g.close()


@pytest.mark.parametrize("lin8", [False, True], ids=["hs_k_lin", "hs_k_lin8"])
@pytest.mark.parametrize("kind", pc.BA_KINDS)
@pytest.mark.parametrize("shape", pc.BA_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ba_device_against_model(shape, kind, lin8):
    s, cv, params, g, kernel, _ = device_ba_case(*shape, kind, lin8)
    rg = g.residuals()
    active = (rg["state"] == 0) & rg["active"].astype(bool)
    o = pc.oracle_at(s, cv, params)
    assert np.array_equal(o.residuals()["state"] == 0, active)   # the oracle sums the same residuals
    if kind == "calib":
        K0 = np.array([s.K[0, 0], s.K[1, 1], s.K[0, 2], s.K[1, 2]])
        assert np.abs(cv * fm.CALIB_SCALE - K0).max() > 0.01 and active.sum() >= 4
    else:
        assert active.mean() >= 0.5
    m = fm.ba_systems(s, active, **pc.model_inputs(s, cv))
    HA, bA = g.system(0)
    Hsc, bsc = g.system(2)
    dg = ba_d(dict(HA=HA, bA=bA, Hsc=Hsc, bsc=bsc), m)
    do = ba_d(ba_oracle_systems(o), m)
    for k in BA_SYSTEMS:
        br = bar(do[k], m["n_terms"])
        print(f"{shape[0]}x{shape[1]} {kind} {kernel} {k}: n {m['n_terms']}  d_oracle {do[k]:.2e}  "
              f"d_device {dg[k]:.2e}  bar {br:.2e}")
    for k in BA_SYSTEMS:
        assert do[k] <= CAP and dg[k] <= bar(do[k], m["n_terms"]), (k, do[k], dg[k])
    g.close()
