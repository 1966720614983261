"""The UseFAST branch of FeatureDetector::ExtractFeatures in numpy, written from the text of include/hs_extract.h
("The FAST branch, as arithmetic"): cv::FAST 9-16 with strict 3x3 suppression, the order (descending response, ties
in raster order), Ssc with its fp64 bracket and binary search, and the final pass.  Integer arithmetic except where
the header says fp64 / float32; the device is held to it bit for bit.  The blur, the angles and the descriptors of the
keys are extract_ref's."""
import math

import numpy as np

import extract_ref

BORDER = extract_ref.BORDER
F = np.float32

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
        (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]

DEFAULTS = dict(threshold=8, num_features=3000, min_dist=5, tolerance=0.1)


def score_plane(img):
    """s of the header for every pixel with a full ring, (H, W) int64; -256 elsewhere (never above a threshold)."""
    I = np.asarray(img, np.uint8).astype(np.int64)
    H, W = I.shape
    s = np.full((H, W), -256, np.int64)
    if H < 7 or W < 7:
        return s
    c = I[3:H - 3, 3:W - 3]
    d = np.stack([c - I[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] for dx, dy in RING])
    best = np.full(c.shape, -256, np.int64)
    for k in range(16):
        arc = d[[(k + j) % 16 for j in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
    s[3:H - 3, 3:W - 3] = best
    return s


def response_plane(img, t):
    s = score_plane(img)
    return np.where(s > t, s - 1, 0)


def corners(img, t):
    """(xy (n, 2) int64, response (n,) int64) of the kept corners in raster order."""
    s = score_plane(img)
    is_corner = s > t
    r = np.where(is_corner, s - 1, 0)
    H, W = r.shape
    p = np.pad(r, 1)
    keep = is_corner.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= r > p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    ys, xs = np.nonzero(keep)          # raster order
    return np.stack([xs, ys], axis=1).astype(np.int64), r[ys, xs]


def order(response):
    """Indices that sort by descending response; equal responses keep their (raster) order."""
    return np.argsort(-np.asarray(response, np.int64), kind="stable")


def c_round(v):
    """C's round: half away from zero."""
    return math.copysign(math.floor(abs(v) + 0.5), v)


def bracket(W, H, n, num_features, tol):
    """(low, high, Kmin, Kmax) of Src/Detector.cpp:457-474 for n >= 2 corners (cols = W, rows = H)."""
    K = min(num_features, n)
    exp1 = H + W + 2 * K
    exp2 = 4 * W + 4 * K + 4 * H * K + H * H + W * W - 2 * H * W + 4 * H * W * K
    exp3 = math.sqrt(float(exp2))
    exp4 = float(K - 1)
    sol1 = -c_round((exp1 + exp3) / exp4)
    sol2 = -c_round((exp1 - exp3) / exp4)
    high = int(sol1 if sol1 > sol2 else sol2)      # truncates
    low = int(math.floor(math.sqrt(float(n // K))))
    Kf, tf = F(K), F(tol)
    kt = F(Kf * tf)
    Kmin = int(c_round(float(F(Kf - kt))))
    Kmax = int(c_round(float(F(Kf + kt))))
    return low, high, Kmin, Kmax


def evaluate(xy, W, H, w):
    """One Ssc evaluation at width w over corners (n, 2) in order: the indices taken."""
    nrows, ncols = 2 * H // w, 2 * W // w
    covered = np.zeros((nrows + 1, ncols + 1), bool)
    out = []
    for i, (x, y) in enumerate(xy.tolist()):
        r, c = 2 * y // w, 2 * x // w
        if covered[r, c]:
            continue
        out.append(i)
        covered[max(r - 2, 0):r + 3, max(c - 2, 0):c + 3] = True
    return out


def ssc(xy, W, H, num_features=3000, tol=0.1):
    """Ssc's search over corners (n, 2) in sorted order.  Returns dict(taken = indices into xy, width = the width whose
    result was taken (-1: none evaluated), counts = [(width, count)] of every evaluation in order, exit = one of
    'empty', 'single', 'found', 'repeat', 'crossed')."""
    n = len(xy)
    if n == 0:
        return dict(taken=[], width=-1, counts=[], exit="empty")
    if n == 1:
        return dict(taken=[0], width=-1, counts=[], exit="single")
    low, high, Kmin, Kmax = bracket(W, H, n, num_features, tol)
    prev, width, taken, counts = -1, -1, [], []
    while True:
        w = low + int((high - low) / 2)            # C division truncates
        if w == prev:
            why = "repeat"
            break
        if low > high:
            why = "crossed"
            break
        taken = evaluate(xy, W, H, w)
        width = w
        counts.append((w, len(taken)))
        if Kmin <= len(taken) <= Kmax:
            why = "found"
            break
        if len(taken) < Kmin:
            high = w - 1
        else:
            low = w + 1
        prev = w
    return dict(taken=taken, width=width, counts=counts, exit=why)


def final(xy, W, H, min_dist=5):
    """The final pass over taken corners (m, 2) in order: the indices kept."""
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    kept = []
    kxy = np.zeros((len(xy), 2), np.int64)
    for i, (x, y) in enumerate(xy.tolist()):
        if x < BORDER or x > W - BORDER or y < BORDER or y > H - BORDER:
            continue
        if np.any(np.abs(kxy[:len(kept)] - (x, y)).max(axis=1) <= min_dist):
            continue
        kxy[len(kept)] = (x, y)
        kept.append(i)
    return kept


def detect(img, params=None):
    """Everything before the descriptors: dict(corner_xy, corner_response (sorted order), ssc = ssc()'s dict,
    xy (n, 2) float32, response (n,) float32)."""
    p = dict(DEFAULTS, **(params or {}))
    H, W = np.asarray(img).shape
    cxy, cr = corners(img, p["threshold"])
    o = order(cr)
    cxy, cr = cxy[o], cr[o]
    s = ssc(cxy, W, H, p["num_features"], p["tolerance"])
    t = np.asarray(s["taken"], np.int64)
    txy, tr = cxy[t], cr[t]
    k = np.asarray(final(txy, W, H, p["min_dist"]), np.int64)
    return dict(corner_xy=cxy.astype(F), corner_response=cr.astype(F), ssc=s,
                xy=txy[k].reshape(-1, 2).astype(F), response=tr[k].astype(F))


def extract_fast(img, pattern, params=None):
    """One ExtractFeatures with UseFAST = true: detect()'s dict plus angle, desc, ambiguous, blurred."""
    out = detect(img, params)
    out["blurred"] = extract_ref.blur(img)
    out["angle"] = extract_ref.angles(img, out["xy"])
    out["desc"], out["ambiguous"] = extract_ref.descriptors(out["blurred"], out["xy"], out["angle"], pattern)
    return out
