"""A plain fp64 model of the Gauss-Newton solve and of the step it applies: EnergyFunctional::solveSystemF,
orthogonalize, System::getNullspaces, resubstituteF_MT and System::doStepFromBackup.  numpy only; nothing here comes
from oracle/ or from the product library (se3_exp, se3_from_data and se3_mul are fp64_model's).

Written from the reference with the settings the project runs -- SOLVER_FIX_LAMBDA, SOLVER_ORTHOGONALIZE_X_LATER and
the LDLT branch:

* solveSystemF, Src/EnergyFunctional.cpp:705-817:
    lambda = 1e-5                                                                       (:708)
    bM_top = bM + HM * getStitchedDeltaF()                                              (:728)
    HFinal = HL + HM + HA,  b = bL + bM_top + bA - b_sc                                 (:756-757)
    HFinal(i, i) *= (1 + lambda)                                                        (:762)
    HFinal -= H_sc * (1.0f / (1 + lambda))                                              (:763)
  `1.0f / (1 + lambda)`: lambda is a double, so the float literal 1.0f is promoted and the quotient is the fp64
  1 / (1 + 1e-5); H_sc is multiplied by it (not divided by 1 + lambda).
    SVecI = 1 / sqrt(diag(HFinal) + 10)                                                 (:799)
    x = SVecI * ldlt(SVecI HFinal SVecI).solve(SVecI * b)                               (:800-801)
    iteration >= 2: orthogonalize(&x, 0)                                                (:804-808)
  Eigen's LDLT<MatrixXX> is LDLT<MatrixXX, Lower>: ldlt() reads the lower triangle of HFinalScaled and never the
  strictly upper one.  That is part of the statement, because the reference's H_sc is not symmetric: the Schur
  stitch fills blocks (i, j) and (j, i) from separately accumulated fp32 sums and copies over the calibration rows
  only, so the two triangles differ at the 1e-7 level and so would x.  (A system read back already mirrored is
  unaffected: the device's stitch and the oracle's accumulateSC both hand over H_sc's upper triangle mirrored,
  DESIGN.md section 5, *Which triangle of H_sc*.)
  The model solves the lower triangle's symmetric matrix with numpy.linalg.solve (LAPACK's pivoted LU), not with
  an LDLT: what remains between it and an implementation is the rounding of the factorization, n 2^-52
  cond(S HFinal S) relative in the scaled unknown.
* orthogonalize, :648-702: N's columns are the 6 pose and 1 scale nullspaces, each normalized (:669-671);
  Npi = U diag(1 / s_i if s_i > solverModeDelta * s_max else 0) V^T of the thin SVD (:676-688);
  x -= 0.5 (N Npi^T + Npi N^T) x (:689-692).
* getStitchedDeltaF, :842-847, of setDeltaF, :128-152: calibration rows value_minus_value_zero cast to float (:140),
  frame rows (state - state_zero).head<8>() (:143).
* the nullspaces: FrameOptimizationData::setStateZero, Include/Frame.h:151-182 (central differences of
  log((evalPT exp(+-eps)) evalPT^-1) with eps = 1e-3, and of the translation scaled by 1.00001^+-1, both over 2e-3),
  stacked by System::getNullspaces, Src/FullSystemOptimize.cpp:616-670, with SCALE_XI_TRANS_INVERSE on the
  translation rows and SCALE_XI_ROT_INVERSE on the rotation rows (:637-638, :663-664; Include/GlobalTypes.h:35-50).
* the step: resubstituteF_MT, Src/EnergyFunctional.cpp:222-247 (calib step = -x.head<4>(), frame step.head<8>() =
  -x.segment<8>(), step.tail<2>() = 0); doStepFromBackup, Src/FullSystemOptimize.cpp:214-231, with all factors 1
  (value = value_backup + step, state = state_backup + step, idepth = idepth_zero = idepth_backup + step);
  FrameOptimizationData::setState, Include/Frame.h:184-197 (PRE_worldToCam = exp(scaled state.head<6>()) evalPT).
* the point step: resubstituteFPt, Src/EnergyFunctional.cpp:249-274: b = bdSumF - xc . Hcd - sum xAd . JpJdF,
  step = -b HdiF, 0 for a point without an active residual.  The model states its result as the minimiser over the
  point's depth of the same quadratic at the frame step x: step = -(bd - H_fp x) / Hdd, with H_fp, Hdd, bd from the
  photometric model (fp64_model.ba_systems' Hfp, Hpp, bp), so nothing of the adjoint bookkeeping is restated.

Mutants (keyword `mutant`) are deliberate errors for the tests' sensitivity checks; None is the model.
"""
from __future__ import annotations

import numpy as np

from fp64_model import se3_exp, se3_from_data, se3_mul

LAMBDA = 1e-5                                    # SOLVER_FIX_LAMBDA, Src/EnergyFunctional.cpp:708
# Include/GlobalTypes.h:35-41 (float literals, all exact in fp64): translation, rotation, a, b (x2)
STATE_SCALE = np.array([0.5, 0.5, 0.5, 1.0, 1.0, 1.0, 10.0, 1000.0, 10.0, 1000.0])
SCALE_XI_TRANS_INVERSE = float(np.float32(1.0) / np.float32(0.5))
SCALE_XI_ROT_INVERSE = float(np.float32(1.0) / np.float32(1.0))
NNS = 7                                          # 6 pose + 1 scale


# ----------------------------------------------------------------------------------------------- SE3 pieces
def se3_inverse(T):
    R, t = T
    return R.T, -(R.T @ t)


def se3_log(T):
    """(upsilon, omega) of T = (R, t): omega = log R, upsilon = V(omega)^-1 t (Sophus' SE3::log)."""
    R, t = T
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])    # sin(th) axis
    s, c = np.linalg.norm(w), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, c)
    om = w * (1.0 + th * th / 6 + 7 * th ** 4 / 360) if th < 1e-4 else w * (th / s)
    O = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    if th < 1e-2:   # (1 - th sin th / (2 (1 - cos th))) / th^2, its series where the quotient cancels
        k = 1.0 / 12 + th * th / 720 + th ** 4 / 30240
    else:
        k = (1.0 - th * np.sin(th) / (2 * (1 - np.cos(th)))) / (th * th)
    Vi = np.eye(3) - 0.5 * O + k * (O @ O)
    return np.concatenate([Vi @ t, om])


# ----------------------------------------------------------------------------------------------- nullspaces
def frame_nullspaces(evalPT):
    """setStateZero's (nullspaces_pose [6, 6] (columns), nullspaces_scale [6]) of one frame, evalPT = (R, t)."""
    Ei = se3_inverse(evalPT)
    pose = np.zeros((6, 6))
    for i in range(6):
        eps = np.zeros(6)
        eps[i] = 1e-3
        lp = se3_log(se3_mul(se3_mul(evalPT, se3_exp(eps)), Ei))
        lm = se3_log(se3_mul(se3_mul(evalPT, se3_exp(-eps)), Ei))
        pose[:, i] = (lp - lm) / 2e-3
    R, t = evalPT
    lp = se3_log(se3_mul((R, t * 1.00001), Ei))
    lm = se3_log(se3_mul((R, t / 1.00001), Ei))
    return pose, (lp - lm) / 2e-3


def nullspaces(evalPT7):
    """System::getNullspaces' pose (6) and scale (1) vectors as the columns of N [4 + 8 nF, 7], from the frames'
    evalPT [nF, 7] (Sophus data order).  The affine nullspaces are formed by the reference too but orthogonalize
    does not use them (Src/EnergyFunctional.cpp:657-662)."""
    evalPT7 = np.asarray(evalPT7, np.float64)
    nF = len(evalPT7)
    N = np.zeros((4 + 8 * nF, NNS))
    for f in range(nF):
        pose, scale = frame_nullspaces(se3_from_data(evalPT7[f]))
        r = 4 + 8 * f
        N[r:r + 6, :6] = pose
        N[r:r + 6, 6] = scale
        N[r:r + 3] *= SCALE_XI_TRANS_INVERSE
        N[r + 3:r + 6] *= SCALE_XI_ROT_INVERSE
    return N


def projector_factors(N, solverModeDelta, mutant=None):
    """orthogonalize's (N with normalized columns, Npi)."""
    N = np.asarray(N, np.float64)
    if mutant == "orth_raw_N":                      # un-normalised columns, no pseudo-inverse
        return N, N.copy()
    Nn = N / np.linalg.norm(N, axis=0)[None, :]
    U, sv, Vt = np.linalg.svd(Nn, full_matrices=False)
    inv = np.where(sv > solverModeDelta * sv.max(), 1.0 / sv, 0.0)
    return Nn, (U * inv[None, :]) @ Vt


def projector(N, solverModeDelta, mutant=None):
    """0.5 (N Npi^T + Npi N^T)."""
    Nn, Npi = projector_factors(N, solverModeDelta, mutant)
    NNpiT = Nn @ Npi.T
    return 0.5 * (NNpiT + NNpiT.T)


# ----------------------------------------------------------------------------------------------- the solve
def stitched_delta(state, state_zero, calib_value, calib_value_zero, mutant=None):
    """getStitchedDeltaF: float32(value - value_zero) | (state - state_zero)[:, :8] per frame."""
    dc = (np.asarray(calib_value, np.float64) - np.asarray(calib_value_zero, np.float64)).astype(np.float32)
    if mutant == "calib_delta_sign":
        dc = -dc
    df = (np.asarray(state, np.float64) - np.asarray(state_zero, np.float64))[:, :8]
    return np.concatenate([dc.astype(np.float64), df.ravel()])


def final_system(HA, bA, HL, bL, Hsc, bsc, HM, bM, delta, mutant=None):
    """(HFinal, b) of solveSystemF's non-orthogonalizing branch."""
    lam = LAMBDA
    H = HL + HM + HA
    bM_top = bM + (0.0 if mutant == "drop_HM_delta" else HM @ delta)
    b = (0.0 if mutant == "drop_bL" else bL) + bM_top + bA + (bsc if mutant == "plus_bsc" else -bsc)
    H = H.copy()
    di = np.diag_indices(len(b))
    inv = float(np.float32(1.0)) / (1 + lam)       # 1.0f / (1 + lambda), evaluated in double
    if mutant == "lambda_on_hsc_diag":             # the damping applied after the Schur term is taken off
        H = H - Hsc * inv
        H[di] *= (1 + lam)
        return H, b
    H[di] *= (1 + lam)
    H = H - Hsc * ((1 + lam) if mutant == "hsc_times" else inv)
    return H, b


def scaling(HFinal):
    return 1.0 / np.sqrt(np.diag(HFinal) + 10.0)


def lower_mirrored(A):
    """The symmetric matrix an LDLT of A's lower triangle factors."""
    L = np.tril(A)
    return L + np.tril(A, -1).T


def scaled_cond(HFinal):
    """cond_2(S HFinal S) of the matrix the LDLT factors."""
    S = scaling(HFinal)
    return float(np.linalg.cond(lower_mirrored(S[:, None] * HFinal * S[None, :])))


def solve_x(HA, bA, HL, bL, Hsc, bsc, HM, bM, delta, N, iteration, solverModeDelta, mutant=None):
    """solveSystemF's x (lastX)."""
    H, b = final_system(HA, bA, HL, bL, Hsc, bsc, HM, bM, delta, mutant)
    S = scaling(H)
    x = S * np.linalg.solve(lower_mirrored(S[:, None] * H * S[None, :]), S * b)
    if iteration >= (1 if mutant == "orth_from_1" else 2):
        x = x - projector(N, solverModeDelta, mutant) @ x
    return x


# ----------------------------------------------------------------------------------------------- the step
def apply_step(state, x, evalPT7, calib):
    """(state_new [nF, 10], [PRE_worldToCam (R, t) per frame], calib_new [4]) of resubstituteF_MT's steps applied by
    doStepFromBackup(1, 1, 1, 1, 1)."""
    state = np.asarray(state, np.float64)
    x = np.asarray(x, np.float64)
    nF = len(state)
    step = np.zeros((nF, 10))
    step[:, :8] = -x[4:].reshape(nF, 8)
    new = state + step
    poses = [se3_mul(se3_exp((STATE_SCALE * new[f])[:6]), se3_from_data(evalPT7[f])) for f in range(nF)]
    return new, poses, np.asarray(calib, np.float64) + (-x[:4])


def point_steps(Hfp, Hpp, bp, x, has_active):
    """(step [nP], scale [nP]): the points' depth steps at the frame step x, step_p = -(bd_p - H_fp,p x) / Hdd_p for
    a point with an active residual and 0 otherwise; scale = (|bd_p| + sum_k |H_fp,pk x_k|) / Hdd_p is the same sum
    with every term's absolute value (the metric's denominator)."""
    x = np.asarray(x, np.float64)
    has = np.asarray(has_active).astype(bool) & (Hpp > 0)
    inv = np.where(has, 1.0 / np.where(has, Hpp, 1.0), 0.0)
    return -(bp - Hfp @ x) * inv, (np.abs(bp) + np.abs(Hfp) @ np.abs(x)) * inv
