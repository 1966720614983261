"""Seeded two-view scenes for the two-view fit's tests: 640 x 480, K = (280, 280, 320, 240), keys of a first frame and
their matches in a second frame under a known motion.  Unless `clean`, every scene has 0.5 px noise, 20 % gross outliers
and (above 8 keys) some keys with status 0.  No image, no file: numpy only."""
import functools

import numpy as np

W, H = 640, 480
K4 = (280.0, 280.0, 320.0, 240.0)
KINDS = ("general", "planar", "rotation", "outlier", "degenerate")


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


R_TRUE = rodrigues([0.02, -0.03, 0.015])
T_TRUE = np.array([-0.24, 0.04, 0.06])
T_TRUE = 0.25 * T_TRUE / np.linalg.norm(T_TRUE)


@functools.lru_cache(maxsize=None)
def scene(kind, n, seed=0, clean=False):
    """dict(xy1, xy2 (n, 2) float32, status (n,) uint8, R, t: the generating motion, outlier (n,) bool)."""
    assert kind in KINDS
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    fx, fy, cx, cy = K4
    xy1 = np.stack([rng.uniform(20, W - 20, n), rng.uniform(20, H - 20, n)], 1)
    if kind == "degenerate":           # three quarters of the keys on one image line
        on_line = np.arange(n) % 4 != 3
        xy1[on_line, 1] = 0.25 * xy1[on_line, 0] + 100.0
    depth = np.full(n, 3.0) if kind == "planar" else rng.uniform(1.5, 6.0, n)
    X = np.stack([(xy1[:, 0] - cx) / fx * depth, (xy1[:, 1] - cy) / fy * depth, depth], 1)
    R = R_TRUE
    t = np.zeros(3) if kind == "rotation" else T_TRUE
    X2 = X @ R.T + t
    xy2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1)
    outlier = np.zeros(n, bool)
    status = np.ones(n, np.uint8)
    if not clean:
        xy1 = xy1 + rng.normal(0, 0.5, (n, 2)) * (0 if kind == "degenerate" else 1)
        xy2 = xy2 + rng.normal(0, 0.5, (n, 2))
        outlier = rng.uniform(size=n) < (1.0 if kind == "outlier" else 0.2)
        rand = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)
        xy2 = np.where(outlier[:, None], rand, xy2)
        if n > 8:
            lost = rng.uniform(size=n) < 0.1
            lost[rng.permutation(n)[:8]] = False      # at least 8 keys stay
            lost[rng.integers(0, n)] = True           # and at least one goes
            if (~lost).sum() < 8:
                lost[:] = False
            status = (~lost).astype(np.uint8)
            xy2 = np.where(lost[:, None], rand[::-1], xy2)
    return dict(kind=kind, n=n, xy1=xy1.astype(np.float32), xy2=xy2.astype(np.float32), status=status, R=R, t=t,
                outlier=outlier, K4=K4)


@functools.lru_cache(maxsize=None)
def sets_of(kind, n, n_sets, seed=0, clean=False):
    """mvSets (n_sets, 8) int32 by the reference's draw; for the degenerate scene at least 6 of every set's 8 keys lie on
    the line."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "h-slam_amd"))
    from hslam_amd.twoview import draw_sets
    s = scene(kind, n, seed, clean)
    rng = np.random.default_rng([seed, n, n_sets, 77])
    if kind != "degenerate":
        return draw_sets(n_sets, s["status"], rng)
    live = np.flatnonzero(s["status"] != 0)
    line = live[live % 4 != 3]
    if len(line) < 6:
        return draw_sets(n_sets, s["status"], rng)
    out = np.zeros((n_sets, 8), np.int32)
    for i in range(n_sets):
        a = rng.permutation(line)[:6]
        rest = np.setdiff1d(live, a)
        out[i] = np.concatenate([a, rng.permutation(rest)[:2]])
    return out


def rotation_angle(Ra, Rb):
    c = (np.trace(np.asarray(Ra, np.float64).reshape(3, 3).T @ np.asarray(Rb, np.float64).reshape(3, 3)) - 1) / 2
    Rd = np.asarray(Ra, np.float64).reshape(3, 3).T @ np.asarray(Rb, np.float64).reshape(3, 3)
    s = np.linalg.norm([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]]) / 2
    return float(np.arctan2(s, c))


def direction_error(ta, tb):
    ta, tb = np.asarray(ta, np.float64), np.asarray(tb, np.float64)
    return float(1 - ta @ tb / (np.linalg.norm(ta) * np.linalg.norm(tb)))
