"""The fp64 model of the tracker and BA systems (tests/fp64_model.py) against the CPU oracle, on the photometric
cases of tests/photo_cases.py.

Metric: d = max_ij |X - X64| / A_ij over entries with A_ij > 0, A the same sum with every term replaced by its
absolute value.  fp32 rounding puts the oracle near 1e-5; a semantic error (a sign, a dropped term, a wrong
linearization point) puts it near 1.

* model against oracle: d <= CAP = 1e-3 on every case and every system (a condition, not a measurement);
* sensitivity: every mutant of the model moves d above 10 x CAP on the cases that exercise it, so the cap cannot hide
  such an error;
* the numeric differentiation is converged: halving the step moves no entry of H by more than 1e-7 of its A.
"""
import functools

import numpy as np
import pytest

import fp64_model as fm
import photo_cases as pc

CAP = 1e-3
BA_SYSTEMS = ("HA", "bA", "Hsc", "bsc")


def ba_oracle_systems(o):
    HA, bA = o.accumulate(0)
    Hsc, bsc = o.accumulate(2)
    return dict(HA=HA, bA=bA, Hsc=Hsc, bsc=bsc)


def ba_d(X, m, A=None):
    """d of the four systems X (dict) against the model output m, normalised by A's (default m's own) A_*."""
    A = m if A is None else A
    return {k: fm.metric(X[k], m[k], A["A_" + k]) for k in BA_SYSTEMS}


@functools.lru_cache(maxsize=None)
def ba_case(n_frames, n_points, kind):
    """(scene, calib value or None, params or None, oracle at that state) of a BA case.  'calib': the oracle's own
    state after one GN step under the weak calibration prior."""
    from oracle_ffi import default_params
    s = pc.make_photo_ba(n_frames, n_points, kind)
    if kind != "calib":
        return s, None, None, pc.oracle_at(s)
    params = pc.calib_params(default_params())
    s2, cv = pc.stepped(s, pc.oracle_at(s, params=params))
    return s2, cv, params, pc.oracle_at(s2, cv, params)


@functools.lru_cache(maxsize=None)
def track_case(name):
    from oracle_ffi import OracleTracker
    s, aff = pc.make_photo_track(name)
    o = OracleTracker(s.width, s.height, s.K4, s.n_levels)
    o.set_scene(s)
    return s, aff, o


def track_poses(s):
    """The poses a tracker case is evaluated at: the truth (r ~ 0) and a perturbed one (r, Huber and cutoff live)."""
    T_true = (fm.se3_from_data(s.T_true))
    R, t = fm.se3_mul(fm.se3_exp([0.004, -0.003, 0.002, 0.002, 0.001, -0.002]), T_true)
    from hslam_amd.scene import se3_data
    return {"truth": np.asarray(s.T_true, np.float64), "perturbed": se3_data(R, t)}


def tracker_model(s, o, lvl, T7, aff, params, **kw):
    return fm.tracker_system(s.new_pyr[lvl], o.pc(lvl), s.K4, lvl, T7, aff, s.ref_aff,
                             (s.ref_exposure, s.new_exposure), params.huberTH, params.coarseCutoffTH, **kw)


def tracker_d(Ho, bo, H, b, A_H, A_b):
    """(d_H, d_b) of a calcGSSSE output against the model's unscaled system, the reference's scale vector applied
    here: (1, 1, 1, 0.5, 0.5, 0.5, 10, 1000) in the output's column order -- SCALE_XI_ROT lands on the translation
    columns and SCALE_XI_TRANS on the rotation columns (fp64_model's approximation 7)."""
    S = fm.TRACKER_SCALE
    SS = np.outer(S, S)
    return fm.metric(Ho, H * SS, A_H * SS), fm.metric(bo, b * S, A_b * S)


# ------------------------------------------------------------------------------------------- model against oracle
@pytest.mark.parametrize("name", list(pc.TRACK_CASES))
def test_tracker_model_against_oracle(name):
    s, aff, o = track_case(name)
    for which, T7 in track_poses(s).items():
        for lvl in range(s.n_levels):
            _, Ho, bo, nw = o.calc_res(lvl, T7, aff, o.params.coarseCutoffTH)
            H, b, A_H, A_b, n = tracker_model(s, o, lvl, T7, aff, o.params)
            assert (n + 3) // 4 * 4 == nw and n > 100, (lvl, n, nw)
            dH, db = tracker_d(Ho, bo, H, b, A_H, A_b)
            print(f"{name} {which} level {lvl}: n {n}  d_oracle H {dH:.2e} b {db:.2e}")
            assert dH <= CAP and db <= CAP, (which, lvl, dH, db)


@pytest.mark.parametrize("kind", pc.BA_KINDS)
@pytest.mark.parametrize("shape", pc.BA_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ba_model_against_oracle(shape, kind):
    s, cv, _, o = ba_case(*shape, kind)
    active = o.residuals()["state"] == 0
    if kind == "calib":
        K0 = np.array([s.K[0, 0], s.K[1, 1], s.K[0, 2], s.K[1, 2]])
        assert np.abs(cv * fm.CALIB_SCALE - K0).max() > 0.01 and active.sum() >= 4
    else:
        assert active.mean() >= 0.5       # the window is photo-consistent
    m = fm.ba_systems(s, active, **pc.model_inputs(s, cv))
    d = ba_d(ba_oracle_systems(o), m)
    print(f"{shape[0]}x{shape[1]} {kind}: IN {int(active.sum())}/{len(active)}  d_oracle "
          + "  ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert max(d.values()) <= CAP, d


def test_ba_model_against_oracle_set_calib():
    """The calibration moved off its linearization value alone (CalibHessian::setValue), everything else at rest."""
    s, _, _, _ = ba_case(5, 200, "photo")
    K0 = np.array([s.K[0, 0], s.K[1, 1], s.K[0, 2], s.K[1, 2]], np.float32).astype(np.float64)
    cv = (K0 + np.array([0.8, -0.6, 0.5, -0.4])) / fm.CALIB_SCALE
    o = pc.oracle_at(s, cv)
    active = o.residuals()["state"] == 0
    assert active.mean() >= 0.5
    m = fm.ba_systems(s, active, **pc.model_inputs(s, cv))
    d = ba_d(ba_oracle_systems(o), m)
    print("5x200 set_calib: d_oracle " + "  ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert max(d.values()) <= CAP, d
    # and the offset matters: the model at the linearization value is far from the oracle
    d0 = ba_d(ba_oracle_systems(o), fm.ba_systems(s, active, **pc.model_inputs(s, None)), m)
    assert max(d0.values()) > 10 * CAP, d0


# ------------------------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("mutant", ["flip_pose_column", "drop_b_from", "exposure_ratio"])
@pytest.mark.parametrize("name", list(pc.TRACK_CASES))
def test_tracker_mutants_clear_the_cap(name, mutant):
    """Both tracker cases have t_ref != t_new and b_ref != 0, so each of these errors is live at every level."""
    s, aff, o = track_case(name)
    T7 = track_poses(s)["perturbed"]
    for lvl in range(s.n_levels):
        _, Ho, bo, _ = o.calc_res(lvl, T7, aff, o.params.coarseCutoffTH)
        _, _, A_H, A_b, _ = tracker_model(s, o, lvl, T7, aff, o.params)
        H, b, _, _, n = tracker_model(s, o, lvl, T7, aff, o.params, mutant=mutant)
        d = max(tracker_d(Ho, bo, H, b, A_H, A_b))
        print(f"{name} level {lvl} {mutant}: kept {n}  d {d:.2e}")
        assert d > 10 * CAP, (lvl, d)


@pytest.mark.parametrize("mutant", ["flip_pose_column", "drop_b_from", "exposure_ratio", "geometry_at_current_state",
                                    "swap_adjoint"])
@pytest.mark.parametrize("shape", pc.BA_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ba_mutants_clear_the_cap(shape, mutant):
    """On photo_fej (exposures, affine states and state - state_zero all live) every mutant moves both the frame
    system and the Schur system."""
    s, cv, _, o = ba_case(*shape, "photo_fej")
    active = o.residuals()["state"] == 0
    m = fm.ba_systems(s, active, **pc.model_inputs(s, cv))
    d = ba_d(ba_oracle_systems(o), fm.ba_systems(s, active, mutant=mutant, **pc.model_inputs(s, cv)), m)
    print(f"{shape[0]}x{shape[1]} {mutant}: " + "  ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert max(d["HA"], d["bA"]) > 10 * CAP and max(d["Hsc"], d["bsc"]) > 10 * CAP, d


def test_fej_mutant_is_silent_without_an_offset():
    """With state == state_zero the linearization point is the current state: the photo case cannot see the FEJ
    mutant (which is why photo_fej exists)."""
    s, cv, _, o = ba_case(5, 200, "photo")
    active = o.residuals()["state"] == 0
    m = fm.ba_systems(s, active, **pc.model_inputs(s, cv))
    mm = fm.ba_systems(s, active, mutant="geometry_at_current_state", **pc.model_inputs(s, cv))
    assert all(np.array_equal(m[k], mm[k]) for k in BA_SYSTEMS)


# ------------------------------------------------------------------------------------------- numeric step
def test_numeric_step_is_converged():
    s, aff, o = track_case("trk320")
    T7 = track_poses(s)["perturbed"]
    H1, _, A1, _, _ = tracker_model(s, o, 0, T7, aff, o.params, step=1e-6)
    H2, _, _, _, _ = tracker_model(s, o, 0, T7, aff, o.params, step=5e-7)
    assert np.abs(H1 - H2).max() <= 1e-7 * np.abs(H1).max() and fm.metric(H2, H1, A1) <= 1e-7
    sb, cv, _, ob = ba_case(5, 200, "photo_fej")
    active = ob.residuals()["state"] == 0
    m1 = fm.ba_systems(sb, active, step=1e-6, **pc.model_inputs(sb, cv))
    m2 = fm.ba_systems(sb, active, step=5e-7, **pc.model_inputs(sb, cv))
    for k in ("HA", "Hsc"):
        assert np.abs(m1[k] - m2[k]).max() <= 1e-7 * np.abs(m1[k]).max(), k
        assert fm.metric(m2[k], m1[k], m1["A_" + k]) <= 1e-7, k
