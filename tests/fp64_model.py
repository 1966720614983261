"""A plain fp64 model of the two Gauss-Newton systems of the photometric energy: the CoarseTracker's 8x8 system
and the BA window's frame / Schur systems.  numpy only; nothing here comes from oracle/ or from the product library.

The model is written from the definition of the energy, not from the reference's operation order:

    r = I_to(pi(T x)) - (a_rel * c_from + b_rel),   a_rel = exp(a_to - a_from) * t_to / t_from,
                                                    b_rel = b_to - a_rel * b_from
    H = sum J^T W J,   b = sum J^T W r

with pi projected in fp64, the three image channels (I, dI/dx, dI/dy) interpolated bilinearly in fp64, every
geometric derivative a central difference of the model's own projection function and every photometric-parameter
derivative a central difference of the model's own residual function.  The unknowns are perturbed directly (a twist
xi under T <- exp(xi) T for the tracker; the 4 calibration values, the 8 `state` entries of a frame and a point's
idepth for the BA), so scale factors, the left-multiplicative exp(S delta) evalPT parametrization and the
host / target adjoints come out of the differences and not out of a formula.

The reference's deliberate approximations are part of the model:

1. The image derivative is the interpolated gradient channel, not the derivative of the interpolant
   (Src/CoarseTracker.cpp:422, 445-446 hitColor[1..2]; Src/OptimizationClasses.cpp:153, 174-180 hitColor[1..2]).
2. In the BA the geometric Jacobian of the pattern's centre pixel serves all 8 pattern pixels
   (Src/OptimizationClasses.cpp:75-76: one projectPoint(u, v, ..., 0, 0, ...) in front of the pattern loop at 141).
3. The weights (Huber x gradient weight) are constants of the linearization
   (Src/OptimizationClasses.cpp:163-175 w, hw; Src/CoarseTracker.cpp:425 hw).
4. First-estimate Jacobians: the geometry is differentiated at evalPT / idepth_zero (PRE_RTll_0, PRE_tTll_0,
   efPoint->idepth_zero, Src/OptimizationClasses.cpp:59, 75-76) and the photometric parameters at state_zero
   (PRE_b0_mode, Src/OptimizationClasses.cpp:38, 65; aff_g2l_0 in EnergyFunctional::setAdjointsF,
   Src/EnergyFunctional.cpp:45-49), while the image is sampled and the residual formed at the current state
   (PRE_KRKiTll, PRE_KtTll, PRE_aff_mode, Src/OptimizationClasses.cpp:37, 144-154).  A GN step moves a point's
   idepth_zero along with its idepth (System::doStepFromBackup, Src/FullSystemOptimize.cpp:208, 230), so only a
   window handed over with idepth != idepth_zero sees the difference.
5. The calibration is not first-estimate: the centre projection and its derivatives use the current camera values
   (HCalib->fxl() etc. inside projectPoint, Include/DirectProjection.h:20-38, and in d_C_x / d_C_y,
   Src/OptimizationClasses.cpp:89-95).
6. The tracker divides its sums by the number of warped terms padded to a multiple of 4
   (Src/CoarseTracker.cpp:454, 309-310 `1.0f/n`), and a term whose |r| exceeds the cutoff is left out
   (Src/CoarseTracker.cpp:428).
7. The tracker's output scale labels are crossed: calcGSSSE multiplies the first three columns (the translation
   part of the twist) by SCALE_XI_ROT and the next three (rotation) by SCALE_XI_TRANS
   (Src/CoarseTracker.cpp:312-321).  The model returns the unscaled system; tests apply TRACKER_SCALE outside.

`A_*` are the same sums with every term replaced by its absolute value; d = max |X - X64| / A over entries with A > 0
is the metric the tests use (fp32 rounding sits near 1e-5 there, a wrong sign or a dropped term near 1).

Mutants (keyword `mutant`) are deliberate errors for the tests' sensitivity checks; None is the model.
"""
from __future__ import annotations

import numpy as np

PATTERN = np.array([[0, -2], [-1, -1], [1, -1], [-2, 0], [0, 0], [2, 0], [-1, 1], [0, 2]], np.float64)

# FrameHessian::setState: state_scaled = S * state (translation, rotation, a, b), Include/Frame.h:184-195
STATE_SCALE = np.array([0.5, 0.5, 0.5, 1.0, 1.0, 1.0, 10.0, 1000.0])
CALIB_SCALE = np.array([50.0, 50.0, 50.0, 50.0])   # CalibHessian::setValue, Include/CalibData.h:77-85
# calcGSSSE's output scaling in the output's column order (approximation 7)
TRACKER_SCALE = np.array([1.0, 1.0, 1.0, 0.5, 0.5, 0.5, 10.0, 1000.0])


# ----------------------------------------------------------------------------------------------- SE3, fp64
def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(xi):
    """(R, t) of exp(xi), xi = (upsilon, omega): R = exp(omega^), t = V upsilon."""
    xi = np.asarray(xi, np.float64)
    ups, om = xi[:3], xi[3:6]
    th = np.linalg.norm(om)
    O = _hat(om)
    if th < 1e-5:
        A, B, Cc = 1.0 - th * th / 6, 0.5 - th * th / 24, 1.0 / 6 - th * th / 120
    else:
        A, B, Cc = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    R = np.eye(3) + A * O + B * (O @ O)
    V = np.eye(3) + B * O + Cc * (O @ O)
    return R, V @ ups


def se3_from_data(d):
    """(R, t) of Sophus data order (qx, qy, qz, qw, tx, ty, tz)."""
    d = np.asarray(d, np.float64)
    x, y, z, w = d[:4] / np.linalg.norm(d[:4])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R, d[4:7].copy()


def se3_mul(a, b):
    return a[0] @ b[0], a[0] @ b[1] + a[1]


def bilinear3(img, x, y):
    """The three channels of img (h, w, 3) at (x, y), bilinear, fp64."""
    img = np.asarray(img)
    ix = np.floor(x).astype(np.int64)
    iy = np.floor(y).astype(np.int64)
    dx = (x - ix)[..., None]
    dy = (y - iy)[..., None]
    p00 = img[iy, ix].astype(np.float64)
    p01 = img[iy, ix + 1].astype(np.float64)
    p10 = img[iy + 1, ix].astype(np.float64)
    p11 = img[iy + 1, ix + 1].astype(np.float64)
    return (1 - dx) * (1 - dy) * p00 + dx * (1 - dy) * p01 + (1 - dx) * dy * p10 + dx * dy * p11


def rel_aff(a_from, b_from, a_to, b_to, t_from, t_to, mutant=None):
    """(a_rel, b_rel) of the energy's brightness transfer from -> to."""
    ratio = t_from / t_to if mutant == "exposure_ratio" else t_to / t_from
    a_rel = np.exp(a_to - a_from) * ratio
    b_rel = b_to - (0.0 if mutant == "drop_b_from" else a_rel * b_from)
    return a_rel, b_rel


def huber_weight(r, th):
    ar = np.abs(r)
    return np.where(ar < th, 1.0, th / np.maximum(ar, 1e-300))


# ----------------------------------------------------------------------------------------------- tracker
def level_K(K4, lvl):
    """CoarseTracker::makeK: the intrinsics of pyramid level lvl (Src/CoarseTracker.cpp:84-89)."""
    fx, fy, cx, cy = (float(x) for x in K4)
    s = float(1 << lvl)
    return fx / s, fy / s, (cx + 0.5) / s - 0.5, (cy + 0.5) / s - 0.5


def _trk_project(T, K, x, y, idepth):
    fx, fy, cx, cy = K
    R, t = T
    ray = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], 0)
    p = R @ ray + t[:, None] * idepth[None, :]
    return fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy, idepth / p[2]


def tracker_system(image, pc, K4, lvl, T7, aff, ref_aff, exposures, huberTH, cutoff, step=1e-6, mutant=None):
    """calcRes + calcGSSSE's 8x8 system, unscaled: (H[8,8], b[8], A_H, A_b, n_kept).
    image: the new frame's level (h, w, 3); pc: dict(u, v, idepth, color) of the level's reference points;
    K4: level-0 (fx, fy, cx, cy); T7: refToNew; aff / ref_aff: (a, b) of the new / reference frame;
    exposures: (t_ref, t_new)."""
    h, w = image.shape[:2]
    K = level_K(K4, lvl)
    x, y = pc["u"].astype(np.float64), pc["v"].astype(np.float64)
    idp, col = pc["idepth"].astype(np.float64), pc["color"].astype(np.float64)
    T = se3_from_data(T7)
    t_ref, t_new = float(exposures[0]), float(exposures[1])

    def residual(I, a, b):
        a_rel, b_rel = rel_aff(ref_aff[0], ref_aff[1], a, b, t_ref, t_new, mutant)
        return I - (a_rel * col_k + b_rel)

    Ku, Kv, nid = _trk_project(T, K, x, y, idp)
    ok = (Ku > 2) & (Kv > 2) & (Ku < w - 3) & (Kv < h - 3) & (nid > 0)
    x, y, idp, col_k, Ku, Kv = x[ok], y[ok], idp[ok], col[ok], Ku[ok], Kv[ok]
    hit = bilinear3(image, Ku, Kv)
    r = residual(hit[:, 0], aff[0], aff[1])
    keep = np.isfinite(hit[:, 0]) & ~(np.abs(r) > cutoff)
    x, y, idp, col_k, hit, r = x[keep], y[keep], idp[keep], col_k[keep], hit[keep], r[keep]
    n = len(r)
    J = np.zeros((n, 8))
    for k in range(6):
        e = np.zeros(6)
        e[k] = step
        up, vp, _ = _trk_project(se3_mul(se3_exp(e), T), K, x, y, idp)
        um, vm, _ = _trk_project(se3_mul(se3_exp(-e), T), K, x, y, idp)
        J[:, k] = hit[:, 1] * (up - um) / (2 * step) + hit[:, 2] * (vp - vm) / (2 * step)
    J[:, 6] = (residual(hit[:, 0], aff[0] + step, aff[1]) - residual(hit[:, 0], aff[0] - step, aff[1])) / (2 * step)
    sb = step * 1e3
    J[:, 7] = (residual(hit[:, 0], aff[0], aff[1] + sb) - residual(hit[:, 0], aff[0], aff[1] - sb)) / (2 * sb)
    if mutant == "flip_pose_column":
        J[:, 4] = -J[:, 4]
    wgt = huber_weight(r, huberTH)
    n_pad = max((n + 3) // 4 * 4, 4)   # no term kept: all sums are 0
    Jw = J * wgt[:, None]
    H = Jw.T @ J / n_pad
    b = Jw.T @ r / n_pad
    A_H = np.abs(Jw).T @ np.abs(J) / n_pad
    A_b = np.abs(Jw).T @ np.abs(r) / n_pad
    return H, b, A_H, A_b, n


# ----------------------------------------------------------------------------------------------- BA window
def _frame_pose(evalPT, s6):
    """exp(S state) evalPT."""
    return se3_mul(se3_exp(STATE_SCALE[:6] * s6), evalPT)


def _ba_project(K, Th, Tt, x, y, idepth):
    """Pixels (x, y) with inverse depth idepth of the host frames Th into the target frames Tt (batched)."""
    fx, fy, cx, cy = K
    Rh, th = Th
    Rt, tt = Tt
    R = Rt @ np.swapaxes(Rh, -1, -2)
    t = tt - np.einsum("...ij,...j->...i", R, th)
    ray = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], -1)
    p = np.einsum("...ij,...j->...i", R, ray) + t * idepth[..., None]
    return fx * p[..., 0] / p[..., 2] + cx, fy * p[..., 1] / p[..., 2] + cy


def ba_systems(scene, active, state=None, idepth=None, idepth_zero=None, calib_value=None, huberTH=9.0,
               outlierTHSumComponent=2500.0, idepth_prior=None, step=1e-6, mutant=None):
    """The BA window's systems in hs_ba_get_system's layout (4 calibration + 8 per frame):
    dict(HA, bA, Hsc, bsc, A_HA, A_bA, A_Hsc, A_bsc, n_terms, and the point blocks Hfp [nP, dim], Hpp [nP], bp [nP]).
    scene: a BAScene (frames_eval, frames_state_zero, frames_exposure, pyramids, pt_*, res_*);
    active [n_res]: the residuals that are active and IN; state [nF, 10], idepth [n], calib_value [4] (unscaled,
    K = 50 * value): the current state (default: the scene's frames_state, pt_idepth and float32(K) / 50);
    idepth_zero [n]: the points' linearization depths (default the scene's; a GN step moves them with idepth,
    System::doStepFromBackup, Src/FullSystemOptimize.cpp:171-260);
    idepth_prior [n]: the points' depth-prior Hessians (default none)."""
    nF = scene.n_frames
    dim = 4 + 8 * nF
    state = np.asarray(scene.frames_state if state is None else state, np.float64)
    state0 = np.asarray(scene.frames_state_zero, np.float64)
    idp = np.asarray(scene.pt_idepth if idepth is None else idepth).astype(np.float64)
    idp0 = np.asarray(scene.pt_idepth_zero if idepth_zero is None else idepth_zero).astype(np.float64)
    if calib_value is None:
        K = scene.K
        calib_value = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32).astype(np.float64) / CALIB_SCALE
    calib_value = np.asarray(calib_value, np.float64)
    expo = np.asarray(scene.frames_exposure, np.float64)
    evalPT = [se3_from_data(d) for d in scene.frames_eval]
    act = np.nonzero(np.asarray(active).astype(bool))[0]
    rp, rt = scene.res_point[act], scene.res_target[act]
    rh = scene.pt_host[rp]
    m = len(act)
    u, v = scene.pt_u[rp].astype(np.float64), scene.pt_v[rp].astype(np.float64)
    color = scene.pt_color[rp].astype(np.float64)
    wpt = scene.pt_weights[rp].astype(np.float64)

    def poses(s):
        P = [_frame_pose(evalPT[f], s[f, :6]) for f in range(nF)]
        return np.stack([p[0] for p in P]), np.stack([p[1] for p in P])

    # ---- residual and weights: image sampled at the current state
    Rc, tc = poses(state)
    Kc = calib_value * CALIB_SCALE
    xs, ys = u[:, None] + PATTERN[None, :, 0], v[:, None] + PATTERN[None, :, 1]
    Ku, Kv = _ba_project(Kc, (Rc[rh][:, None], tc[rh][:, None]), (Rc[rt][:, None], tc[rt][:, None]), xs, ys,
                         np.broadcast_to(idp[rp][:, None], xs.shape))
    hit = np.zeros((m, 8, 3))
    for f in range(nF):
        sel = rt == f
        if sel.any():
            hit[sel] = bilinear3(scene.pyramids[f][0], Ku[sel], Kv[sel])

    def residual(sh, st):
        """r [m, 8] with the host's / target's (state[6], state[7]) = sh / st ([m, 2] each)."""
        a_rel, b_rel = rel_aff(STATE_SCALE[6] * sh[:, 0], STATE_SCALE[7] * sh[:, 1], STATE_SCALE[6] * st[:, 0],
                               STATE_SCALE[7] * st[:, 1], expo[rh], expo[rt], mutant)
        return hit[..., 0] - (a_rel[:, None] * color + b_rel[:, None])

    r = residual(state[rh, 6:8], state[rt, 6:8])
    wg = np.sqrt(outlierTHSumComponent / (outlierTHSumComponent + hit[..., 1] ** 2 + hit[..., 2] ** 2))
    wg = 0.5 * (wg + wpt)
    W = wg * wg * huber_weight(r, huberTH)

    # ---- geometry: central differences of the centre projection at evalPT / idepth_zero / the current calibration
    lin_state = state if mutant == "geometry_at_current_state" else np.zeros_like(state)
    lin_idp = idp if mutant == "geometry_at_current_state" else idp0

    def centre(cv, sh6, st6, d):
        Ph = [_frame_pose(evalPT[f], lin_state[f, :6]) for f in range(nF)]
        Rl, tl = np.stack([p[0] for p in Ph]), np.stack([p[1] for p in Ph])
        Rh, th, Rt, tt = Rl[rh], tl[rh], Rl[rt], tl[rt]
        if sh6 is not None:   # exp(S (s + e)) evalPT, the same e for every residual's host
            Ph = [_frame_pose(evalPT[f], lin_state[f, :6] + sh6) for f in range(nF)]
            Rh, th = np.stack([p[0] for p in Ph])[rh], np.stack([p[1] for p in Ph])[rh]
        if st6 is not None:
            Pt = [_frame_pose(evalPT[f], lin_state[f, :6] + st6) for f in range(nF)]
            Rt, tt = np.stack([p[0] for p in Pt])[rt], np.stack([p[1] for p in Pt])[rt]
        return np.stack(_ba_project(cv * CALIB_SCALE, (Rh, th), (Rt, tt), u, v, d), -1)

    # local parameter order: calibration 0..3, host state 4..11, target state 12..19, idepth 20
    G = np.zeros((m, 2, 21))
    d0 = lin_idp[rp]
    for k in range(4):
        e = np.zeros(4)
        e[k] = step
        G[:, :, k] = (centre(calib_value + e, None, None, d0) - centre(calib_value - e, None, None, d0)) / (2 * step)
    for k in range(6):
        e = np.zeros(6)
        e[k] = step
        G[:, :, 4 + k] = (centre(calib_value, e, None, d0) - centre(calib_value, -e, None, d0)) / (2 * step)
        G[:, :, 12 + k] = (centre(calib_value, None, e, d0) - centre(calib_value, None, -e, d0)) / (2 * step)
    G[:, :, 20] = (centre(calib_value, None, None, d0 + step) - centre(calib_value, None, None, d0 - step)) / (2 * step)
    if mutant == "flip_pose_column":
        G[:, :, 12 + 4] = -G[:, :, 12 + 4]
    if mutant == "swap_adjoint":
        G[:, :, 4:10], G[:, :, 12:18] = G[:, :, 12:18].copy(), G[:, :, 4:10].copy()

    # ---- the Jacobian rows: image gradient x geometry, and the photometric parameters at state_zero
    J = np.einsum("mic,mcp->mip", hit[..., 1:3], G)
    sh0, st0 = state0[rh, 6:8], state0[rt, 6:8]
    for k in range(2):
        e = np.zeros(2)
        e[k] = step
        J[:, :, 4 + 6 + k] = (residual(sh0 + e, st0) - residual(sh0 - e, st0)) / (2 * step)
        J[:, :, 12 + 6 + k] = (residual(sh0, st0 + e) - residual(sh0, st0 - e)) / (2 * step)

    # ---- per-residual 21 x 21 blocks, then the window's systems
    JW = J * W[..., None]
    M = np.einsum("mip,miq->mpq", JW, J)
    g = np.einsum("mip,mi->mp", JW, r)
    AM = np.einsum("mip,miq->mpq", np.abs(JW), np.abs(J))
    Ag = np.einsum("mip,mi->mp", np.abs(JW), np.abs(r))
    idx = np.concatenate([np.broadcast_to(np.arange(4), (m, 4)), 4 + 8 * rh[:, None] + np.arange(8)[None, :],
                          4 + 8 * rt[:, None] + np.arange(8)[None, :]], 1)          # [m, 20] global columns
    out = {}
    for name, Mx, gx in (("", M, g), ("A_", AM, Ag)):
        H = np.zeros((dim, dim))
        b = np.zeros(dim)
        np.add.at(H, (idx[:, :, None], idx[:, None, :]), Mx[:, :20, :20])
        np.add.at(b, idx, gx[:, :20])
        out[name + "HA"], out[name + "bA"] = H, b
    # Schur complement of the points: H_fp (H_pp + prior)^-1 H_pf from the same Jacobian
    nP = scene.n_points
    prior = np.zeros(nP) if idepth_prior is None else np.asarray(idepth_prior, np.float64)
    Hpp = np.zeros(nP)
    np.add.at(Hpp, rp, M[:, 20, 20])
    Hpp = Hpp + prior
    for name, Mx, gx, sign in (("", M, g, 1.0), ("A_", AM, Ag, 0.0)):
        Hfp = np.zeros((nP, dim))
        bp = np.zeros(nP)
        np.add.at(Hfp, (rp[:, None], idx), Mx[:, :20, 20])
        np.add.at(bp, rp, gx[:, 20])
        pd = prior * (idp - idp0)
        bp = bp + (pd if sign else np.abs(pd))
        if sign:   # the point blocks themselves (tests/solve_model.py's point step)
            out["Hfp"], out["Hpp"], out["bp"] = Hfp, Hpp, bp
        has = Hpp > 0
        inv = np.where(has, 1.0 / np.where(has, Hpp, 1.0), 0.0)
        out[name + "Hsc"] = (Hfp * inv[:, None]).T @ Hfp
        out[name + "bsc"] = Hfp.T @ (bp * inv)
    out["n_terms"] = 8 * m
    return out


def metric(X, X64, A):
    """d = max |X - X64| / A over the entries with A > 0."""
    sel = A > 0
    return float((np.abs(np.asarray(X) - X64)[sel] / A[sel]).max())
