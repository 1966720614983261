"""The device's GN solve (hs_k_solve), the step it applies and the point steps against the fp64 model
(tests/solve_model.py), on the windows and variants of tests/test_solve_model.py: make_photo_ba(nF, 40 nF) for
nF = 2 ... 8 (n = 20, 28, ..., 68 = HS_MAXDIM; n / 4 = 5, 7, ..., 17 panels), 160x120, always hs_k_lin.

Granular path: linearizeAll(reset=True), read system(0 / 1 / 2), the marginal prior and the state, then solveSystem(it)
against solve_x on exactly those arrays, so the linearize kernels drop out and what remains is the kernel's assembly
of HFinal / b, its scaling, its LDLT and its orthogonalization.

    bar(d_x), bar(d_blk) = min(max(4 d_oracle, 64 n 2^-52 cond(S HFinal S)), 1e-6)

d_oracle is the CPU oracle's figure for the same window, state and prior, computed in the same test (the oracle's own
systems against the model); 4 x is the project's margin for model bars; 64 x the floor allows a blocked LDLT without
pivoting against LAPACK's pivoted LU.  Each test prints cond, the floor, d_oracle, d_device and the bar.

Applied step (doStepFromBackup): state and calibration equal apply_step's bit for bit (state + (-x) is one fp64 add),
pose7 within 1e-12, idepth == float32(idepth + step) with idepth_zero moved along.
Point steps: points()["step"] against point_steps(the photometric model's H_fp / Hdd / bd, the device's x) at
min(4 d_oracle, 1e-3).
The gauge projector has no read-back, so it is compared through its effect: x(iteration 2) - x(iteration 1) on one
window against -P64 x(iteration 1), P64 from the model's nullspaces; debug_nullspace_error() stays 0.
Fused loop (iterate(it, 1) on a second context, HS_APPLY): the pre-step systems are the granular context's bit for
bit, and the stepped state and calibration equal state + (-x_granular) bit for bit.  (-(state_after - state_before)
itself is not x wherever state_before != 0: the add rounds to state's ulp, so the subtraction returns x rounded
there.  Holding the sum is the exact form of the same claim; where state_before is 0 the two coincide.)
"""
import functools

import numpy as np
import pytest

import fp64_model as fm
import photo_cases as pc
import solve_model as sm
from test_solve_model import (CASES, CEIL, NFS, STEP_CAP, VARIANTS, case_id, metrics, model_x, oracle_case_at,
                              params_of, random_prior, read_inputs, scene_of, step_metric, system_figures)

pytestmark = pytest.mark.gpu

FUSED = [(nF, v) for nF in (2, 5, 8) for v in ("photo_it0", "fej_it2")]


def bar(d_oracle, floor):
    return min(max(4 * d_oracle, 64 * floor), CEIL)


def device_window(n_frames, variant):
    """(window linearized at the variant's state with its prior set, scene, calib value, value_zero, HM, bM)."""
    from hslam_amd._lib import default_params
    from hslam_amd.ba import BAWindow
    kind, _, with_prior, id0 = VARIANTS[variant]
    s = scene_of(n_frames, kind, id0)
    g = BAWindow(s, params=params_of(kind, default_params))
    calib_zero = g.frames()["calib"].copy()          # right after the window is set: value_zero
    g.linearizeAll(reset=True)
    cv = None
    if kind == "calib":   # the device's own state after one GN step under the weak calibration prior
        s, cv = pc.stepped(s, g)
        g.linearizeAll(reset=True)
    assert g.partition()["kernel"] == "hs_k_lin"
    HM, bM = np.zeros((g.dim, g.dim)), np.zeros(g.dim)
    if with_prior:
        HM, bM = random_prior(g.system(0)[0])
        g.set_marginal_prior(HM, bM)
    return g, s, cv, calib_zero, HM, bM


def device_inputs(g, calib_zero):
    HM, bM = g.marginal_prior()
    return read_inputs(g.system, HM, bM, g.frames(), g.frame_eval(), calib_zero, g.params.solverModeDelta)


@functools.lru_cache(maxsize=None)
def device_run(n_frames, variant):
    """One granular GN iteration of the device on a case, everything the tests compare recorded; and the oracle at
    the same state and prior."""
    from oracle_ffi import default_params as oracle_default_params
    kind, iteration, _, _ = VARIANTS[variant]
    g, s, cv, calib_zero, HM, bM = device_window(n_frames, variant)
    inp = device_inputs(g, calib_zero)
    assert np.array_equal(inp["HM"], HM) and np.array_equal(inp["bM"], bM)
    rg = g.residuals()
    out = dict(scene=s, cv=cv, inp=inp, iteration=iteration, active=(rg["state"] == 0) & rg["active"].astype(bool),
               before=g.frames(), evalPT=g.frame_eval()["evalPT"], idepth=g.points()["idepth"].copy(),
               nullspace_error=g.debug_nullspace_error())
    out["x"] = g.solveSystem(iteration)
    out["step"] = g.points()["step"].copy()
    g.doStepFromBackup()
    out["after"] = g.frames()
    out["idepth_after"] = g.points()["idepth"].copy()
    out["idepth_zero_after"] = g.point_state()["idepth_zero"].copy()
    g.close()
    out["oracle"] = oracle_case_at(s, cv, params_of(kind, oracle_default_params), variant, prior=(HM, bM))
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_solve_device_against_model(case):
    r = device_run(*case)
    o = r["oracle"]
    So, _, _ = system_figures(o["inp"])
    do_x, do_blk, _ = metrics(o["x"], model_x(o["inp"], o["iteration"]), So)
    S, cond, floor = system_figures(r["inp"])
    dg_x, dg_blk, which = metrics(r["x"], model_x(r["inp"], r["iteration"]), S)
    bx, bb = bar(do_x, floor), bar(do_blk, floor)
    print(f"{case_id(case)}: n {len(S)}  cond {cond:.2e}  floor {floor:.2e}  d_oracle x {do_x:.2e} blocks {do_blk:.2e}"
          f"  d_device x {dg_x:.2e} blocks {dg_blk:.2e} ({which})  bar x {bx:.2e} blocks {bb:.2e}")
    assert r["nullspace_error"] == 0
    assert np.array_equal(r["inp"]["HA"], r["inp"]["HA"].T) and np.array_equal(r["inp"]["Hsc"], r["inp"]["Hsc"].T)
    assert do_x <= CEIL and do_blk <= CEIL, (do_x, do_blk)
    assert dg_x <= bx and dg_blk <= bb, (dg_x, bx, dg_blk, bb, which)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_applied_step_device_against_model(case):
    r = device_run(*case)
    new, poses, calib = sm.apply_step(r["before"]["state"], r["x"], r["evalPT"], r["before"]["calib"])
    assert np.abs(r["x"]).max() > 0
    assert np.array_equal(r["after"]["state"], new)
    assert np.array_equal(r["after"]["calib"], calib)
    worst = 0.0
    for f, (R, t) in enumerate(poses):
        Rg, tg = fm.se3_from_data(r["after"]["pose"][f])
        worst = max(worst, np.abs(Rg - R).max(), np.abs(tg - t).max())
    print(f"{case_id(case)}: max |pose - exp(S state) evalPT| {worst:.2e}")
    assert worst <= 1e-12
    assert np.array_equal(r["idepth_after"], (r["idepth"] + r["step"]).astype(np.float32))
    assert np.array_equal(r["idepth_zero_after"], r["idepth_after"])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_point_steps_device_against_model(case):
    r = device_run(*case)
    o = r["oracle"]["o"]
    active_o = o.residuals()["state"] == 0
    assert np.array_equal(active_o, r["active"])                # oracle and device step the same points
    d_o, _, _ = step_metric(o.points()["step"], r["scene"], r["cv"], active_o, r["oracle"]["x"])
    d_g, _, has = step_metric(r["step"], r["scene"], r["cv"], r["active"], r["x"])
    br = min(4 * d_o, STEP_CAP)
    print(f"{case_id(case)}: points with an active residual {int(has.sum())}/{len(has)}  d_oracle {d_o:.2e}  "
          f"d_device {d_g:.2e}  bar {br:.2e}")
    assert d_o <= STEP_CAP and d_g <= br, (d_o, d_g, br)
    assert np.all(r["step"][~has] == 0)


@pytest.mark.parametrize("n_frames", NFS)
def test_projector_effect_device_against_model(n_frames):
    """x(iteration 2) - x(iteration 1) on the same systems is -P x(iteration 1) with the model's projector.  The two
    solves run on two contexts of the window (solveSystem consumes the system, and a second linearization of one
    context starts from the frame energy threshold the first one set): their systems are bit-identical.  An entry
    of P off by e moves the difference by up to e ||x||_inf, so 1e-9 ||x||_inf is the read-back comparison's 1e-9
    of P's largest entry (P is a projector: that entry is at most 1)."""
    g, _, _, calib_zero, _, _ = device_window(n_frames, "fej_it2")
    inp = device_inputs(g, calib_zero)
    x1 = g.solveSystem(1)
    g.close()
    g, _, _, calib_zero, _, _ = device_window(n_frames, "fej_it2")
    inp2 = device_inputs(g, calib_zero)
    assert all(np.array_equal(inp[k], inp2[k]) for k in ("HA", "bA", "HL", "bL", "Hsc", "bsc", "HM", "bM", "delta"))
    x2 = g.solveSystem(2)
    assert g.debug_nullspace_error() == 0
    g.close()
    P = sm.projector(inp["N"], inp["solverModeDelta"])
    err = np.abs((x2 - x1) + P @ x1).max()
    print(f"{n_frames} frames: |x2 - x1 + P x1| {err:.2e}  |P x1| {np.abs(P @ x1).max():.2e}  |x1| {np.abs(x1).max():.2e}")
    assert np.abs(P @ x1).max() > 1e-6 * np.abs(x1).max()      # the projection is live
    assert err <= 1e-9 * np.abs(x1).max()


@pytest.mark.parametrize("case", FUSED, ids=case_id)
def test_fused_step_is_the_granular_step(case):
    r = device_run(*case)
    g, _, _, calib_zero, _, _ = device_window(*case)
    inp = device_inputs(g, calib_zero)
    for k in ("HA", "bA", "HL", "bL", "Hsc", "bsc", "HM", "bM", "delta"):
        assert np.array_equal(inp[k], r["inp"][k]), k           # the same pre-step systems, bit for bit
    before = g.frames()
    assert np.array_equal(before["state"], r["before"]["state"]) and np.array_equal(before["calib"], r["before"]["calib"])
    g.iterate(r["iteration"], 1)
    after = g.frames()
    g.close()
    new, _, calib = sm.apply_step(before["state"], r["x"], r["evalPT"], before["calib"])
    assert np.array_equal(after["state"], new)
    assert np.array_equal(after["calib"], calib)
    zero = before["state"][:, :8] == 0                          # there the stepped state is -x itself
    assert zero.any() and np.array_equal(-after["state"][:, :8][zero], r["x"][4:].reshape(-1, 8)[zero])
    assert np.array_equal(after["pose"], r["after"]["pose"])
