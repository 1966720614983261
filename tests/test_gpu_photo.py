"""Device against oracle on the photometric cases (tests/photo_cases.py), at the bars of the existing parity tests:
exposures != 1, affine states far from 0, state != state_zero, a calibration off its linearization value.

* BA, under both linearize kernels: test_gpu_ba.test_linearize_bit_exact's per-residual asserts and its _close_H /
  _close_b on HA / bA and H_sc / b_sc;
* tracker: test_gpu_track.test_calc_res_parity's asserts at every level, and one trackNewestCoarse run per case
  through _lm_divergence at the oracle's own summation-order spread.
"""
import numpy as np
import pytest

import photo_cases as pc
from test_fp64_model import track_case, track_poses
from test_gpu_ba import _close_b, _close_H
from test_gpu_fp64_model import device_ba_case
from test_gpu_track import _close_H as _close_H_trk
from test_gpu_track import _lm_divergence, _order_spread, _pose_err

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lin8", [False, True], ids=["hs_k_lin", "hs_k_lin8"])
@pytest.mark.parametrize("kind", pc.BA_KINDS)
@pytest.mark.parametrize("shape", pc.BA_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ba_photo_parity(shape, kind, lin8):
    s, cv, params, g, _, eg = device_ba_case(*shape, kind, lin8)
    from oracle_ffi import OracleBA
    o = OracleBA(s, params=params)
    if cv is not None:
        o.set_calib(cv)
    eo = o.linearize_all(reset=True)
    o.apply_res()
    rg, ro = g.residuals(), o.residuals()
    assert np.array_equal(rg["state"], ro["state"])
    active_o = ro["state"] == 0
    assert active_o.any()
    assert np.array_equal(rg["active"].astype(bool), active_o)
    assert np.array_equal(rg["energy"], ro["energy"].astype(np.float32))
    assert np.array_equal(rg["energy_wo"], ro["energy_wo"].astype(np.float32))
    assert np.array_equal(rg["JpJdF"][active_o], ro["JpJdF"][active_o])
    assert np.array_equal(rg["center"][active_o], ro["center"][active_o])
    assert abs(eg - eo) <= 1e-9 * abs(eo)
    assert np.array_equal(g.frames()["energyTH"], o.frames()["energyTH"])
    for which in (0, 2):
        Ho, bo = o.accumulate(which)
        Hg, bg = g.system(which)
        okH, rH = _close_H(Hg, Ho)
        okb, rb = _close_b(bg, bo, Ho)
        assert okH, f"which={which} H worst ratio {rH}"
        assert okb, f"which={which} b worst ratio {rb}"
    g.close()


@pytest.fixture(scope="module", params=list(pc.TRACK_CASES))
def photo_pair(request):
    from hslam_amd.track import CoarseTracker
    s, aff, o = track_case(request.param)
    g = CoarseTracker(s.width, s.height, s.K4, s.n_levels)
    g.set_scene(s)
    yield s, aff, g, o
    g.close()


def test_calc_res_photo_parity(photo_pair):
    s, aff, g, o = photo_pair
    for which, T in track_poses(s).items():
        for lvl in range(s.n_levels):
            for cut in (g.params.coarseCutoffTH, 2 * g.params.coarseCutoffTH):
                rg, Hg, bg, ng = g.calcRes(lvl, T, aff, cut)
                ro, Ho, bo, no = o.calc_res(lvl, T, aff, cut)
                assert ng == no and rg[1] == ro[1], (which, lvl, cut)
                assert round(rg[5] * rg[1]) == round(ro[5] * ro[1])
                assert abs(rg[0] - ro[0]) <= 2e-5 * abs(ro[0]) + 1e-3
                for k in (2, 4):
                    assert abs(rg[k] - ro[k]) <= 1e-4 * abs(ro[k]) + 1e-6
                assert _close_H_trk(Hg, Ho), (which, lvl, np.abs(Hg - Ho).max())
                sb = np.abs(bo).max() + 1e-30
                assert np.all(np.abs(bg - bo) <= 1e-4 * (np.abs(bo) + 1e-3 * sb))


def test_track_photo_parity(photo_pair):
    """trackNewestCoarse from a pose and an affine estimate near the consistent ones: the LM log agrees with the
    oracle's up to a near-tie, then the final pose / affine at test_gpu_track.test_track_parity's bars."""
    s, aff, g, o = photo_pair
    T0 = track_poses(s)["perturbed"]
    aff0 = [aff[0] + 0.02, aff[1] + 1.0]
    minRes = np.full(5, np.nan)
    okg, Tg, ag = g.trackNewestCoarse(T0, aff0, s.n_levels - 1, minRes)
    spread = _order_spread(o, T0, aff0, s.n_levels - 1, minRes)
    ro = o.track(T0, aff0, s.n_levels - 1, minRes)
    assert okg == ro["ok"] and okg
    k = _lm_divergence(g.lm_log(0), o.lm_log(), spread)
    tol_T, tol_a, tol_b = (min(max(1e-5, 10 * spread[2]), 1e-4), 1e-5, 1e-3) if k is None else (2e-3, 1e-2, 0.5)
    print(f"pose bar {tol_T:.2e} (oracle order spread {spread[2]:.2e}), first near-tie {k}")
    assert _pose_err(Tg, ro["T"]) < tol_T, k
    assert abs(ag[0] - ro["aff"][0]) < tol_a and abs(ag[1] - ro["aff"][1]) < tol_b, k
    assert _pose_err(Tg, s.T_true) < 1e-2
