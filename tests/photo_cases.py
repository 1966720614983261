"""Scenes that light up the photometric terms: exposures != 1, affine states far from 0, state != state_zero.

Built on hslam_amd.scene's generators (whose defaults stay as they are).  A frame's level-0 image I becomes
g I + beta with g = t e^a and beta = b for an exposure t and an affine state (a, b); the pyramid, the points' colours
and their gradient weights are rebuilt from the new image the way make_ba_scene builds them, so the window stays
photo-consistent: r = I_t' - a_rel c' - b_rel = g_t (I_t - c).
"""
from __future__ import annotations

import copy
import math

import numpy as np

K640 = np.array([[256.0, 0, 319.5], [0, 254.4, 239.5], [0, 0, 1.0]])

# (frames, points) of the BA windows: with lane = (point, target slot) 8 frames fill 7 of hs_k_lin8's 8 slots, 5 frames
# leave half of them empty, 2 frames all but one
BA_SHAPES = [(2, 64), (5, 200), (8, 240)]
BA_KINDS = ["photo", "photo_fej", "calib"]
# width, height, levels, points, (t_ref, t_new), ref_aff
TRACK_CASES = {"trk160": (160, 120, 3, 300, (0.7, 1.3), (-0.2, -4.0)),
               "trk320": (320, 240, 4, 400, (1.0, 1.3), (0.1, 5.0))}


def scaled_K(width):
    """The 640-wide default intrinsics at another width (pixel centres kept: c' = (c + 0.5) s - 0.5)."""
    s = width / 640.0
    K = K640.copy()
    K[0, 0] *= s
    K[1, 1] *= s
    K[0, 2] = (K[0, 2] + 0.5) * s - 0.5
    K[1, 2] = (K[1, 2] + 0.5) * s - 0.5
    return K


def relight(scene, t, a, b):
    """The BAScene with frame i exposed t[i] and re-lit by g = t e^a, beta = b; state = state_zero = (a / 10, b / 1000)."""
    from hslam_amd.scene import PATTERN, make_dir_pyramid
    s = copy.copy(scene)
    g = (np.asarray(t) * np.exp(np.asarray(a))).astype(np.float32)
    s.pyramids = [make_dir_pyramid(g[i] * scene.pyramids[i][0][..., 0] + np.float32(b[i]), scene.n_levels)
                  for i in range(scene.n_frames)]
    col = np.zeros_like(scene.pt_color)
    wgt = np.zeros_like(scene.pt_weights)
    for h in range(scene.n_frames):
        sel = np.nonzero(scene.pt_host == h)[0]
        if len(sel) == 0:
            continue
        py = scene.pt_v[sel].astype(np.int64)[:, None] + PATTERN[None, :, 1]
        px = scene.pt_u[sel].astype(np.int64)[:, None] + PATTERN[None, :, 0]
        smp = s.pyramids[h][0][py, px]
        gx, gy = smp[..., 1], smp[..., 2]
        c2500 = np.float32(2500.0)
        col[sel] = smp[..., 0]
        wgt[sel] = np.sqrt(c2500 / (c2500 + (gx * gx + gy * gy))).astype(np.float32)
    s.pt_color, s.pt_weights = col, wgt
    s.frames_exposure = np.asarray(t, np.float32)
    st = np.zeros((scene.n_frames, 10))
    st[:, 6] = np.asarray(a) / 10.0
    st[:, 7] = np.asarray(b) / 1000.0
    s.frames_state, s.frames_state_zero = st, st.copy()
    return s


def make_photo_ba(n_frames, n_points, kind="photo", seed=5):
    """160x120 window of n_frames x n_points.  kind: 'photo' (exposures in [0.6, 1.6], |a| <= 0.3, |b| <= 12,
    state == state_zero), 'photo_fej' (the same with pose / affine state offsets from state_zero and idepth 1 % off
    idepth_zero) or 'calib' (the photo window; the caller takes one GN step under calib_params, see stepped).
    The pose / depth noise is half make_ba_scene's default: at 160 px it leaves three quarters of the residuals IN."""
    from hslam_amd.scene import make_ba_scene
    base = make_ba_scene(n_points=n_points, n_frames=n_frames, width=160, height=120, K=scaled_K(160), seed=seed,
                         pose_noise=(0.002, 0.001), idepth_noise=0.005)
    rng = np.random.default_rng(seed + 101)
    t = rng.uniform(0.6, 1.6, n_frames)
    a = rng.uniform(-0.3, 0.3, n_frames)
    b = rng.uniform(-12.0, 12.0, n_frames)
    a[-1], b[-1] = 0.3, -12.0      # the ranges' ends are in every window
    s = relight(base, t, a, b)
    if kind == "photo_fej":
        st = s.frames_state.copy()
        st[1:, :6] += rng.normal(size=(n_frames - 1, 6)) * 2e-3
        st[1:, 6:8] += rng.normal(size=(n_frames - 1, 2)) * 1e-3
        s.frames_state = st
        s.pt_idepth = (s.pt_idepth_zero * (1.0 + 0.01 * rng.choice([-1.0, 1.0], s.n_points))).astype(np.float32)
    return s


CALIB_PRIOR = 1e5   # initialCalibHessian of the 'calib' windows (default 5e9): one GN step moves the camera by pixels


def calib_params(params):
    """The BA parameters with the calibration prior weak enough for one GN step to move the camera values."""
    p = type(params)()
    for name, _ in params._fields_:
        setattr(p, name, getattr(params, name))
    p.initialCalibHessian = CALIB_PRIOR
    return p


def stepped(scene, w):
    """(scene', calib value) after one GN iteration of `w` (a BAWindow or an OracleBA on `scene`, linearized): the
    window whose frames_state, frames_energyTH and idepths are w's, so that another engine starts from exactly that
    state.  The calibration is then off its linearization value (the scene's K), poses and affine parameters off
    state_zero; idepth_zero moves with idepth (System::doStepFromBackup, Src/FullSystemOptimize.cpp:171-260)."""
    w.iterate(0, 1)
    fr = w.frames()
    s = copy.copy(scene)
    s.frames_state = fr["state"].copy()
    s.frames_energyTH = fr["energyTH"].copy()
    s.pt_idepth = w.points()["idepth"].copy()
    s.pt_idepth_zero = s.pt_idepth.copy()
    return s, fr["calib"].copy()


def oracle_at(scene, calib_value=None, params=None):
    """The oracle on `scene` at `calib_value` (None: the scene's K), linearized with its residuals applied."""
    from oracle_ffi import OracleBA
    o = OracleBA(scene, params=params)
    if calib_value is not None:
        o.set_calib(calib_value)
    o.linearize_all(reset=True)
    o.apply_res()
    return o


def model_inputs(scene, calib_value=None):
    """ba_systems' keyword arguments for `scene` at `calib_value`."""
    return dict(state=scene.frames_state, idepth=scene.pt_idepth, idepth_zero=scene.pt_idepth_zero,
                calib_value=calib_value)


def make_photo_track(name):
    """The TrackScene of TRACK_CASES[name] and the new frame's aff that keeps the pair consistent:
    a_new = a_true + a_ref - ln(t_new / t_ref), b_new = b_true + e^a_true b_ref."""
    from hslam_amd.scene import make_track_scene
    w, h, levels, n, (t_ref, t_new), ref_aff = TRACK_CASES[name]
    s = make_track_scene(n_points=n, width=w, height=h, K=scaled_K(w), n_levels=levels)
    s.ref_exposure, s.new_exposure = t_ref, t_new
    s.ref_aff = np.array(ref_aff, np.float64)
    a_true, b_true = s.aff_true
    aff = np.array([a_true + ref_aff[0] - math.log(t_new / t_ref), b_true + math.exp(a_true) * ref_aff[1]])
    return s, aff
