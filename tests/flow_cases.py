"""Inputs of the keypoint-flow tests (tests/test_flow.py, tests/test_gpu_flow.py) and the reference results they
share: each reference call is computed once per process and never modified."""
import functools

import numpy as np
from scipy import ndimage

import flow_ref as ref

MARGIN = 20
SHIFT_CASES = (((96, 80), (2.5, -1.25)), ((64, 48), (-5.25, 3.5)), ((61, 61), (-3.0, 1.75)), ((96, 80), (1.5, 0.75)))
COVERAGE_SIZES = ((96, 80), (64, 48), (61, 61), (30, 30))
INIT_OFFSET = np.array([1.5, -0.5], np.float32)
# (image seed, point seed) per coverage size.  "error window outside" needs a point whose last step carries it out of
# the image: about one point in a thousand.  These seeds were picked on the reference so that three of the four sizes
# hold one (tests/test_flow.py asserts that every exit reason occurs).
COVERAGE_SEEDS = ((33, 42), (31, 41), (32, 41), (32, 40))


def field(w, h, seed):
    """Gaussian-filtered (sigma 2) normal noise scaled to 0..255, float64, with a 20 px margin still on"""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.standard_normal((h + 2 * MARGIN, w + 2 * MARGIN)), 2.0)
    return (f - f.min()) / (f.max() - f.min()) * 255.0


def crop8(f):
    return np.ascontiguousarray(np.rint(f[MARGIN:-MARGIN, MARGIN:-MARGIN]).astype(np.uint8))


def image_pair(w, h, shift, seed, patch=0):
    """(first, second): the field and the same field moved by `shift` = (dx, dy) px with a cubic spline; `patch`: side
    of a constant square put in the centre of both"""
    f = field(w, h, seed)
    g = ndimage.shift(f, (shift[1], shift[0]), order=3, mode="nearest")
    a, b = crop8(f), crop8(np.clip(g, 0, 255))
    if patch:
        y0, x0 = (h - patch) // 2, (w - patch) // 2
        a[y0:y0 + patch, x0:x0 + patch] = 128
        b[y0:y0 + patch, x0:x0 + patch] = 128
    return a, b


def interior_points(w, h, n, seed, border=12):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(border, w - border, n), rng.uniform(border, h - border, n)], 1).astype(np.float32)


def coverage_points(w, h, seed, n=300):
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-12, w + 12, n), rng.uniform(-12, h + 12, n)], 1)
    fixed = [(-30, 5), (w + 40, 5), (5, -30), (5, h + 40), (w / 2, h / 2), (0, 0), (w - 1, h - 1)]
    return np.concatenate([pts, np.array(fixed, np.float64)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def shift_case(k):
    """SHIFT_CASES[k]: (first, second, points, shift, reference result)"""
    (w, h), shift = SHIFT_CASES[k]
    a, b = image_pair(w, h, shift, seed=10 + k)
    pts = interior_points(w, h, 200, seed=20 + k)
    return a, b, pts, np.array(shift, np.float32), ref.calc(a, b, pts)


@functools.lru_cache(maxsize=None)
def coverage_inputs(k):
    w, h = COVERAGE_SIZES[k]
    a, b = image_pair(w, h, (1.75, -1.25), seed=COVERAGE_SEEDS[k][0], patch=24)
    return a, b, coverage_points(w, h, seed=COVERAGE_SEEDS[k][1])


@functools.lru_cache(maxsize=None)
def coverage_case(k, with_init=False):
    """COVERAGE_SIZES[k]: (first, second, points, init or None, reference result)"""
    a, b, pts = coverage_inputs(k)
    init = pts + INIT_OFFSET if with_init else None
    return a, b, pts, init, ref.calc(a, b, pts, init)


def chain_frames(w=96, h=80, seed=50):
    """three frames of one field, moved by (0, 0), (2.6, 0.3), (5.1, 0.9): per-frame flows near 2.6 px, whose
    truncating sum differs from the float sum"""
    f = field(w, h, seed)
    out = []
    for dx, dy in ((0, 0), (2.6, 0.3), (5.1, 0.9)):
        out.append(crop8(np.clip(ndimage.shift(f, (dy, dx), order=3, mode="nearest"), 0, 255)))
    return out


@functools.lru_cache(maxsize=None)
def chain_case():
    """(frames, points, [reference Matcher state after track 1, after track 2])"""
    frames = chain_frames()
    pts = np.concatenate([interior_points(96, 80, 120, seed=51), np.array([[-3, 4], [200, 10], [1, 1]], np.float32)])
    m = ref.Matcher(frames[0], pts)
    steps = []
    for img in frames[1:]:
        n_good = m.track(img, 7)
        steps.append(dict(n_good=n_good, xy=m.xy.copy(), prev_xy=m.prev_xy.copy(), good=m.last["good"].copy(),
                          status=m.last["status"].copy(), err=m.last["err"].copy(), iters=int(m.last["iters"].sum()),
                          mean_flow=ref.mean_flow(m.prev_xy, m.xy, m.last["good"])))
    return frames, pts, steps
