"""tests/fast_ref.py, the numpy model of the UseFAST branch (include/hs_extract.h, "The FAST branch, as arithmetic"),
against literal restatements of the definitions it claims, the search bracket against hand-computed values, and the
argument errors of the C entry points that need no device."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import fast_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-slam_amd"))


# ---- the model against the definitions

def brute_corner(I, x, y, b):
    """9 contiguous ring pixels all brighter than I(x, y) by more than b, or all darker by more than b."""
    v = int(I[y, x])
    ring = [int(I[y + dy, x + dx]) for dx, dy in fr.RING] * 2
    for k in range(16):
        arc = ring[k:k + 9]
        if min(arc) > v + b or max(arc) < v - b:
            return True
    return False


def test_response_is_the_largest_threshold_that_still_detects():
    """The segment test holds at threshold b iff s > b, so the largest threshold at which a pixel is still a corner is
    s - 1: the response (cornerScore's value; the first threshold that fails, minus 1).  Checked for every pixel that
    is a corner at t, for the three thresholds the device tests use, and the zero band with it."""
    W, H = 24, 20
    I = np.random.default_rng(4).integers(0, 256, size=(H, W), dtype=np.uint8)
    s = fr.score_plane(I)
    largest = np.full((H, W), -1, np.int64)
    for y in range(3, H - 3):
        for x in range(3, W - 3):
            for b in range(254, -1, -1):
                if brute_corner(I, x, y, b):
                    largest[y, x] = b
                    break
    n_checked = 0
    for t in (0, 8, 254):
        r = fr.response_plane(I, t)
        band = np.ones((H, W), bool)
        band[3:H - 3, 3:W - 3] = False
        assert np.all(r[band] == 0)
        for y in range(3, H - 3):
            for x in range(3, W - 3):
                is_corner = brute_corner(I, x, y, t)
                assert is_corner == (s[y, x] > t)
                if is_corner:
                    assert r[y, x] == largest[y, x] == s[y, x] - 1 and t <= r[y, x] <= 254
                    n_checked += 1
                else:
                    assert r[y, x] == 0
    assert n_checked > 50


def test_suppression_is_strict_and_raster_ordered():
    I = np.random.default_rng(5).integers(0, 3, size=(40, 45)).astype(np.uint8) * 90   # ties everywhere
    r = fr.response_plane(I, 8)
    xy, resp = fr.corners(I, 8)
    want = []
    for y in range(3, 37):
        for x in range(3, 42):
            nb = [r[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]
            if r[y, x] > max(nb):
                want.append((x, y, r[y, x]))
    assert len(want) > 20
    assert [(x, y, v) for (x, y), v in zip(xy.tolist(), resp.tolist())] == want
    o = fr.order(resp)
    rs = resp[o]
    assert np.all(rs[:-1] >= rs[1:])
    same = rs[:-1] == rs[1:]
    assert same.sum() > 5 and np.all(o[:-1][same] < o[1:][same])   # ties keep raster order


def literal_evaluate(xy, cols, rows, width):
    """Src/Detector.cpp:486-513 restated: fp64 cell size, a boolean grid, clamped ranges."""
    c = width / 2.0
    ncols, nrows = int(math.floor(cols / c)), int(math.floor(rows / c))
    covered = [[False] * (ncols + 1) for _ in range(nrows + 1)]
    result = []
    for i, (x, y) in enumerate(xy):
        row, col = int(math.floor(float(y) / c)), int(math.floor(float(x) / c))
        if not covered[row][col]:
            result.append(i)
            reach = math.floor(width / c)
            r0 = int(row - reach) if row - reach >= 0 else 0
            r1 = int(row + reach) if row + reach <= nrows else nrows
            c0 = int(col - reach) if col - reach >= 0 else 0
            c1 = int(col + reach) if col + reach <= ncols else ncols
            for rr in range(r0, r1 + 1):
                for cc in range(c0, c1 + 1):
                    covered[rr][cc] = True
    return result


@pytest.mark.parametrize("W,H", [(101, 67), (64, 48)])
def test_cell_rule_equals_the_literal_grid(W, H):
    rng = np.random.default_rng(W)
    xy = np.stack([rng.integers(0, W, 400), rng.integers(0, H, 400)], axis=1)
    for w in (1, 2, 3, 5, 7, 12, 13, 31, 64, 135, 203):
        got = fr.evaluate(xy, W, H, w)
        assert got == literal_evaluate(xy.tolist(), W, H, w), w
        # and the rule as the header words it: no corner taken before has a cell within Chebyshev distance 2
        cells = np.stack([2 * xy[:, 1] // w, 2 * xy[:, 0] // w], axis=1)
        taken = []
        for i in range(len(xy)):
            if not any(np.abs(cells[i] - cells[j]).max() <= 2 for j in taken):
                taken.append(i)
        assert got == taken, w


def literal_final(xy, cols, rows, min_dist):
    """Src/Detector.cpp:525-551 restated: the occupancy image, the xx > 0 / yy > 0 quirk included."""
    occ = np.zeros((rows, cols), np.uint8)
    kept = []
    for i, (x, y) in enumerate(xy):
        if y > rows - 19 or y < 19 or x > cols - 19 or x < 19:
            continue
        if occ[y, x] == 255:
            continue
        kept.append(i)
        for ki in range(-min_dist, min_dist + 1):
            yy = y + ki
            if 0 < yy < rows:
                for kj in range(-min_dist, min_dist + 1):
                    xx = x + kj
                    if 0 < xx < cols:
                        occ[yy, xx] = 255
    return kept


@pytest.mark.parametrize("min_dist", [0, 1, 5, 40])
def test_final_pass_equals_the_occupancy_image(min_dist):
    W, H = 101, 67
    rng = np.random.default_rng(9)
    xy = np.stack([rng.integers(0, W, 600), rng.integers(0, H, 600)], axis=1)
    xy = xy[np.unique(xy, axis=0, return_index=True)[1].argsort()]    # corners are distinct pixels
    xy = np.concatenate([[[W - 19, H - 19], [W - 18, 30], [30, H - 18], [19, 19], [18, 40], [40, 18]], xy])
    got = fr.final(xy, W, H, min_dist)
    assert got == literal_final(xy.tolist(), W, H, min_dist)
    assert got[0] == 0 and 1 not in got and 2 not in got and 4 not in got and 5 not in got
    if min_dist == 0:
        inside = [i for i, (x, y) in enumerate(xy.tolist()) if 19 <= x <= W - 19 and 19 <= y <= H - 19]
        assert len(got) == len(set(map(tuple, xy[inside].tolist())))


# ---- the bracket

@pytest.mark.parametrize("W,H,n,nf,tol,want", [
    # exp1 = 7120, exp2 = 3692200160, exp3 = 60763.5: sol1 = -23, sol2 = 18; 9000 / 3000 = 3 -> low 1
    (640, 480, 9000, 3000, 0.1, (1, 18, 2700, 3300)),
    # K = n = 500: exp1 = 1168, exp2 = 13671560, exp3 = 3697.5: (1168 - 3697.5) / 499 = -5.07
    (101, 67, 500, 3000, 0.1, (1, 5, 450, 550)),
    # exp1 = 7600, exp2 = 5445691424, exp3 = 73794.9: -22.07; 20000 / 3000 = 6 -> low 2
    (1232, 368, 20000, 3000, 0.1, (2, 22, 2700, 3300)),
    # K = 2: exp1 = 1124, exp2 = 2489608, exp3 = 1577.85: sol2 = 454; 2 - 0.2 = 1.8 -> 2, 2.2 -> 2
    (640, 480, 2, 3000, 0.1, (1, 454, 2, 2)),
    (640, 480, 75000, 2, 0.0, (193, 454, 2, 2)),       # 193^2 = 37249 <= 37500 < 194^2
    # K = 15: 15 * 0.1f rounds to 1.5f, so Kmin = round(13.5) = 14 and Kmax = round(16.5) = 17 (in double: 13, 17);
    # exp1 = 198, exp2 = 411660, exp3 = 641.6: (198 - 641.6) / 14 = -31.7
    (101, 67, 15, 3000, 0.1, (1, 32, 14, 17)),
])
def test_bracket_table(W, H, n, nf, tol, want):
    assert fr.bracket(W, H, n, nf, tol) == want


def test_search_special_cases():
    assert fr.ssc(np.zeros((0, 2), np.int64), 101, 67) == dict(taken=[], width=-1, counts=[], exit="empty")
    assert fr.ssc(np.array([[50, 30]]), 101, 67) == dict(taken=[0], width=-1, counts=[], exit="single")
    s = fr.ssc(np.array([[50, 30], [20, 40]]), 101, 67)
    assert s["taken"] == [0, 1] and s["exit"] == "found" and s["width"] >= 1


# ---- the C entry points' argument errors (no device call is reached)

def test_abi_argument_errors():
    from hslam_amd._lib import hs_fast_params, load
    lib = load()
    p = hs_fast_params()
    lib.hs_fast_params_default(C.byref(p))
    assert (p.threshold, p.num_features, p.min_dist) == (8, 3000, 5) and p.tolerance == np.float32(0.1)
    lib.hs_fast_params_default(None)                      # tolerated
    assert C.sizeof(hs_fast_params) == 16
    n = C.c_int(-7)
    img = np.zeros(64, np.uint8)
    ip = img.ctypes.data_as(C.c_void_p)
    # a null extractor is refused before anything else is looked at; the parameter ranges need a real extractor
    # and are checked on the device (tests/test_gpu_fast.py::test_argument_ranges)
    assert lib.hs_extractor_extract_fast(None, C.byref(p), ip, C.byref(n)) == -1
    assert lib.hs_extractor_extract_fast(None, None, None, None) == -1
    assert lib.hs_extractor_extract_fast_u8(None, C.byref(p), None, ip, C.byref(n)) == -1
    assert lib.hs_extractor_extract_fast_image(None, C.byref(p), None, C.byref(n)) == -1
    assert lib.hs_extractor_get_fast(None, None, None, None, None, None) == -1
    assert b"null" in lib.hs_last_error()
    assert n.value == -7
