"""The corner detector (hs_extractor_extract_fast, hs_k_fast_*) against tests/fast_ref.py, the numpy form of the
contract in include/hs_extract.h.  Corners, their order, Ssc's width and result, the final pass, responses and angles
are integer, fp64 or exactly rounded float32 arithmetic in a fixed order: the bar is array_equal.  Descriptor bits
follow tests/test_gpu_extract.py's rule: every bit the reference does not flag ambiguous must match, and the flagged
share stays within extract_cases.MAX_AMBIGUOUS."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import extract_cases as cases
import extract_ref as ref
import fast_ref as fr

pytestmark = pytest.mark.gpu

W, H = cases.W, cases.H
TILE_W, TILE_H = 64, 16          # hs_k_fast_resp's tile


@pytest.fixture(scope="module")
def pattern():
    return cases.random_pattern()


@pytest.fixture(scope="module")
def ex(pattern):
    from hslam_amd.extract import FeatureExtractor
    e = FeatureExtractor(W, H, (W - 38) * (H - 38), pattern)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def image(kind):
    if kind == "random":
        return cases.random_image()
    if kind == "grey3":        # three grey levels: almost every response ties, so the tie order is what is tested
        return (np.random.default_rng(3).integers(0, 3, size=(H, W)) * 100).astype(np.uint8)
    if kind == "checker":      # 7-px squares
        y, x = np.mgrid[0:H, 0:W]
        return ((((x // 7) + (y // 7)) & 1) * 200 + 20).astype(np.uint8)
    if kind == "constant":
        return np.full((H, W), 77, np.uint8)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def model(kind, threshold=8, num_features=3000, min_dist=5, tolerance=0.1):
    """fast_ref.extract_fast of a named image, computed once per parameter set and never modified."""
    return fr.extract_fast(image(kind), cases.random_pattern(),
                           dict(threshold=threshold, num_features=num_features, min_dist=min_dist, tolerance=tolerance))


def blob(img, px, py, peak=255, rest=200):
    """A bright 3x3 blob whose one strict maximum of response is its centre (px, py)."""
    img[py - 1:py + 2, px - 1:px + 2] = rest
    img[py, px] = peak
    return img


def check_detect(e, want, n=None):
    """Corners in sorted order, the width taken, the keys and their responses."""
    f = e.get_fast()
    assert f["n_corners"] == len(want["corner_xy"])
    assert np.array_equal(f["corner_xy"], want["corner_xy"])
    assert np.array_equal(f["corner_response"], want["corner_response"])
    assert f["width"] == want["ssc"]["width"]
    got = e.get()
    if n is not None:
        assert n == len(want["xy"])
    assert np.array_equal(got["xy"], want["xy"])
    assert np.array_equal(f["response"], want["response"])
    return got


def check_all(e, want, n=None):
    check_detect(e, want, n)
    got = e.get(blurred=True)
    assert np.array_equal(got["blurred"], want["blurred"])
    assert np.array_equal(got["angle"], want["angle"])
    share = cases.ambiguous_share(want)
    assert share <= cases.MAX_AMBIGUOUS, share
    differ = ref.unpack_bits(got["desc"]) != ref.unpack_bits(want["desc"])
    assert not np.any(differ & ~want["ambiguous"]), int(np.sum(differ & ~want["ambiguous"]))
    return got


# ---- corners and responses in sorted order

@pytest.mark.parametrize("t", [0, 8, 254])
@pytest.mark.parametrize("kind", ["random", "grey3", "checker", "constant"])
def test_corners_sorted(ex, kind, t):
    want = model(kind, threshold=t)
    n = ex.extract_fast(image(kind), dict(threshold=t))
    check_detect(ex, want, n)
    if kind == "constant":
        f = ex.get_fast()
        assert n == 0 and f["n_corners"] == 0 and f["width"] == -1
    if kind == "grey3" and t == 8:
        r = want["corner_response"]
        assert len(r) > 100 and len(np.unique(r)) <= 4          # ties are the rule here
    if kind == "random" and t == 8:
        assert len(want["corner_xy"]) > 300 and n > 10
    if kind == "checker":      # an X junction has no arc of 9: step edges everywhere and not one corner
        assert len(want["corner_xy"]) == 0


@pytest.mark.parametrize("px,py", [(3, 3), (W - 4, 3), (3, H - 4), (W - 4, H - 4),          # the first / last pixel with a ring
                                   (2, 30), (W - 3, 30), (40, 2), (40, H - 3),               # inside the zero band
                                   (TILE_W - 1, TILE_H - 1), (TILE_W, TILE_H), (TILE_W + 1, 2 * TILE_H - 1),
                                   (TILE_W - 2, 3 * TILE_H)])                                # across the kernel's tiles
def test_blob_at_ring_band_and_tile_edges(ex, px, py):
    img = np.zeros((H, W), np.uint8)
    x0, x1, y0, y1 = max(px - 1, 0), min(px + 2, W), max(py - 1, 0), min(py + 2, H)
    img[y0:y1, x0:x1] = 200
    img[py, px] = 255
    cxy, cr = fr.corners(img, 8)
    in_band = px < 3 or px > W - 4 or py < 3 or py > H - 4
    assert ([px, py] in cxy.tolist()) == (not in_band)
    want = fr.detect(img)
    ex.extract_fast(img)
    check_detect(ex, want)


# ---- n = 1 and n = 2

@pytest.mark.parametrize("peaks", [[(50, 33)], [(50, 33), (30, 40)]])
def test_one_and_two_corners(ex, pattern, peaks):
    img = np.zeros((H, W), np.uint8)
    for i, (px, py) in enumerate(peaks):
        blob(img, px, py, peak=255 - 20 * i)
    want = fr.extract_fast(img, pattern)
    assert len(want["corner_xy"]) == len(peaks)
    assert want["ssc"]["exit"] == ("single" if len(peaks) == 1 else "found")
    n = ex.extract_fast(img)
    assert n == len(peaks)
    got = check_all(ex, want, n)
    assert got["xy"].tolist() == [list(p) for p in peaks]
    assert (ex.get_fast()["width"] == -1) == (len(peaks) == 1)


# ---- every exit of the search

@pytest.mark.parametrize("kind,nf,tol,exit_,evaluated,more_than_n", [
    ("random", 2, 0.0, "found", True, False),
    ("random", 20, 0.0, "repeat", True, False),
    ("random", 3000, 0.0, "found", True, True),        # num_features > n
    ("random", 3000, 0.1, "found", True, True),
    ("grey3", 30, 0.05, "crossed", True, False),      # low > high after five widths: the last one's result
])
def test_ssc_exits(ex, kind, nf, tol, exit_, evaluated, more_than_n):
    want = model(kind, num_features=nf, tolerance=tol, min_dist=0)
    s = want["ssc"]
    if exit_ is not None:
        assert s["exit"] == exit_                      # the case is the one it was chosen to be
    assert (len(s["counts"]) > 0) == evaluated and (nf > len(want["corner_xy"])) == more_than_n
    n = ex.extract_fast(image(kind), dict(num_features=nf, tolerance=tol, min_dist=0))
    check_detect(ex, want, n)
    # min_dist 0 drops nothing but the border: the keys are the taken corners inside it, so the taken set is checked
    t = want["corner_xy"][np.asarray(s["taken"], np.int64)]
    inside = (t[:, 0] >= 19) & (t[:, 0] <= W - 19) & (t[:, 1] >= 19) & (t[:, 1] <= H - 19)
    assert np.array_equal(ex.get()["xy"], t[inside])


@pytest.mark.parametrize("kind,nf,tol", [("random", 3000, 0.1), ("random", 2, 0.0), ("random", 20, 0.0),
                                         ("grey3", 30, 0.05)])
def test_every_width_of_the_bracket(ex, kind, nf, tol):
    """Each width of [low, high] is evaluated in its own workgroup: the count and the taken indices of every one of
    them against the model's evaluation at that width, and the bracket itself."""
    want = model(kind, num_features=nf, tolerance=tol, min_dist=0)
    cxy = want["corner_xy"].astype(np.int64)
    ex.extract_fast(image(kind), dict(num_features=nf, tolerance=tol, min_dist=0))
    got = ex.fast_widths()
    low, high, _, _ = fr.bracket(W, H, len(cxy), nf, tol)
    assert (got["low"], got["high"]) == (low, high) and high - low >= 3
    assert sorted(got["taken"]) == list(range(low, high + 1))
    for w, taken in got["taken"].items():
        assert taken.tolist() == fr.evaluate(cxy, W, H, w), w
    for w, count in want["ssc"]["counts"]:
        assert len(got["taken"][w]) == count


def test_argument_ranges(ex):
    """Every out-of-range parameter is HS_ERR_INVALID and leaves the current result alone."""
    from hslam_amd._lib import HsError
    from hslam_amd.image import DeviceImage
    n = ex.extract_fast(image("random"))
    before = ex.get()
    im = DeviceImage(W, H, 1)
    for field, bad in [("threshold", -1), ("threshold", 255), ("num_features", 1), ("min_dist", -1),
                       ("tolerance", 1.0), ("tolerance", -0.01), ("tolerance", float("nan"))]:
        with pytest.raises(HsError, match=rf"\(-1\).*{field}"):
            ex.extract_fast(image("random"), {field: bad})
        with pytest.raises(HsError, match=rf"\(-1\).*{field}"):
            ex.extract_fast_image(im, {field: bad})
    from hslam_amd._lib import ptr
    from hslam_amd.extract import fast_params
    p, img = fast_params(), image("random")
    assert ex.lib.hs_extractor_extract_fast(ex.h, None, ptr(img), None) == -1
    assert ex.lib.hs_extractor_extract_fast(ex.h, C.byref(p), None, None) == -1
    assert ex.lib.hs_extractor_extract_fast_u8(ex.h, C.byref(p), None, ptr(img), None) == -1
    assert ex.lib.hs_extractor_extract_fast_image(ex.h, C.byref(p), None, None) == -1
    im.close()
    after = ex.get()
    assert ex.n == n and all(np.array_equal(before[k], after[k]) for k in before)
    # a min_dist beyond the image is the image's size: one key survives
    assert ex.extract_fast(image("random"), dict(min_dist=2 ** 31 - 1)) == 1
    check_detect(ex, model("random", min_dist=max(W, H)))


def test_ssc_bracket_crossed_before_any_width(pattern):
    """A long, low image dense with corners and num_features = 2: low = floor(sqrt(n / 2)) exceeds high, the loop
    breaks before it evaluates a width, and the result is empty."""
    from hslam_amd.extract import FeatureExtractor
    w, h = 3600, 39
    img = cases.random_image(w, h, seed=21)
    want = fr.detect(img, dict(num_features=2))
    s = want["ssc"]
    low, high, _, _ = fr.bracket(w, h, len(want["corner_xy"]), 2, 0.1)
    assert s["exit"] == "crossed" and s["counts"] == [] and low > high and len(want["corner_xy"]) > 10000
    e = FeatureExtractor(w, h, 100, pattern)
    assert e.extract_fast(img, dict(num_features=2)) == 0
    check_detect(e, want, 0)
    assert e.get_fast()["width"] == -1
    e.close()


# ---- the final pass

@pytest.mark.parametrize("min_dist", [0, 5, 40])
def test_final_pass_min_dist(ex, min_dist):
    want = model("random", min_dist=min_dist)
    n = ex.extract_fast(image("random"), dict(min_dist=min_dist))
    check_detect(ex, want, n)
    xy = want["xy"]
    if min_dist and len(xy) > 1:
        d = np.abs(xy[:, None, :] - xy[None, :, :]).max(axis=2) + np.eye(len(xy)) * 1e6
        assert d.min() > min_dist
    counts = [len(model("random", min_dist=m)["xy"]) for m in (0, 5, 40)]
    assert counts[0] > counts[1] > counts[2] >= 1


def test_final_pass_border_is_asymmetric(ex, pattern):
    """Blobs on dim noise (the descriptors need texture), a threshold the noise stays under, and tolerance 0 so that
    Ssc takes all 8 corners and only the final pass drops any."""
    img = np.random.default_rng(101).integers(0, 40, size=(H, W)).astype(np.uint8)
    kept = [(19, 19), (W - 19, H - 19), (W - 19, 30), (45, H - 19)]
    dropped = [(W - 18, 45), (60, H - 18), (18, 40), (70, 18)]
    for i, (px, py) in enumerate(kept + dropped):
        blob(img, px, py, peak=255 - 5 * i)
    params = dict(min_dist=0, tolerance=0.0, threshold=100)
    want = fr.extract_fast(img, pattern, params)
    assert len(want["corner_xy"]) == 8 == len(want["ssc"]["taken"])
    assert sorted(want["xy"].tolist()) == sorted([float(x), float(y)] for x, y in kept)
    n = ex.extract_fast(img, params)
    check_all(ex, want, n)                            # angle and descriptor gathers 18 px from the edge


# ---- angles and descriptors

def test_random_image_angles_and_descriptors(ex):
    want = model("random")
    assert cases.ambiguous_share(want) <= cases.MAX_AMBIGUOUS and len(want["xy"]) > 20
    n = ex.extract_fast(image("random"))
    got = check_all(ex, want, n)
    assert len(np.unique(got["desc"], axis=0)) > 0.9 * n
    want0 = model("random", min_dist=0)               # more keys: nothing thinned but the border
    assert len(want0["xy"]) > 100
    check_all(ex, want0, ex.extract_fast(image("random"), dict(min_dist=0)))


# ---- capacity, interleaving

def test_capacity_exact_and_one_less(pattern):
    from hslam_amd.extract import ExtractOverflow, FeatureExtractor
    want = model("random")
    need = len(want["xy"])
    exact = FeatureExtractor(W, H, need, pattern)
    assert exact.extract_fast(image("random")) == need
    check_all(exact, want)
    exact.close()
    small = FeatureExtractor(W, H, need - 1, pattern)
    m = np.zeros((H, W), np.float32)
    m[30, 30] = m[31, 29] = 1
    for previous in ("map", "fast"):
        if previous == "map":
            assert small.extract(m, cases.random_image(seed=8)) == 2
        else:
            assert small.extract_fast(image("grey3"), dict(min_dist=20)) == len(model("grey3", min_dist=20)["xy"]) < need
        before = small.get(blurred=True)
        fast_before = small.get_fast() if previous == "fast" else None
        with pytest.raises(ExtractOverflow, match=r"\(-1\)") as ei:
            small.extract_fast(image("random"))
        assert ei.value.needed == need
        after = small.get(blurred=True)
        for k in before:
            assert np.array_equal(before[k], after[k]), (previous, k)
        if previous == "fast":
            fast_after = small.get_fast()
            for k in fast_before:
                assert np.array_equal(fast_before[k], fast_after[k]), k
            check_all(small, model("grey3", min_dist=20))
    small.close()


def test_interleaved_with_map_extracts(ex):
    from hslam_amd._lib import HsError
    m, img, pat, want_map = cases.descriptor_case()

    def check_map():
        assert ex.extract(m, img) == len(want_map["xy"])
        got = ex.get(blurred=True)
        for k in ("xy", "angle", "blurred"):
            assert np.array_equal(got[k], want_map[k]), k
        differ = ref.unpack_bits(got["desc"]) != ref.unpack_bits(want_map["desc"])
        assert not np.any(differ & ~want_map["ambiguous"])
        with pytest.raises(HsError, match=r"\(-5\)"):
            ex.get_fast()

    check_map()
    check_all(ex, model("grey3"), ex.extract_fast(image("grey3")))
    check_map()
    check_all(ex, model("random"), ex.extract_fast(image("random")))


def test_get_fast_before_any_extract(pattern):
    from hslam_amd._lib import HsError
    from hslam_amd.extract import FeatureExtractor
    e = FeatureExtractor(W, H, 10, pattern)
    with pytest.raises(HsError, match=r"\(-5\)"):
        e.get_fast()
    e.close()


# ---- the chain

def test_tracer_add_keys_matches_add_points(ex):
    from hslam_amd.trace import ImmatureTracer
    want = model("random", min_dist=0)
    n = ex.extract_fast(image("random"), dict(min_dist=0))
    xy = ex.get()["xy"]
    assert n == len(want["xy"]) > 100
    rng = np.random.default_rng(12)
    host = rng.uniform(0, 255, size=(H, W, 3)).astype(np.float32)
    a = ImmatureTracer(W, H, n + 5)
    b = ImmatureTracer(W, H, n + 5)
    for t in (a, b):
        t.set_host_image(0, host)
    assert a.add_keys(ex, 0) == n
    b.add_points(np.zeros(n, np.int32), xy[:, 0], xy[:, 1])
    pa, pb = a.points(), b.points()
    for k in pa:
        assert pa[k].shape == pb[k].shape and np.array_equal(pa[k], pb[k], equal_nan=True), k
    assert np.any(pa["color"] != 0)
    a.close()
    b.close()


def test_device_image_and_raw_frame_equal_host_image(pattern):
    from hslam_amd.extract import FeatureExtractor
    from hslam_amd.image import DeviceImage
    from hslam_amd.undistort import Undistorter, make_calib
    u = Undistorter(make_calib("Pinhole", W, H, W, H, (0.6 * W, 0.6 * W, 0.5 * W - 0.5, 0.5 * H - 0.5), (0.0,), "none"))
    raw = image("random")
    _, img8 = u.undistort(raw)
    im = DeviceImage(W, H, 1)
    im.set_u8(u, raw)
    a = FeatureExtractor(W, H, 2000, pattern)
    b = FeatureExtractor(W, H, 2000, pattern)
    c = FeatureExtractor(W, H, 2000, pattern)
    na, nb, nc = a.extract_fast(img8), b.extract_fast_image(im), c.extract_fast_u8(u, raw)
    assert na == nb == nc > 10
    ga, fa = a.get(blurred=True), a.get_fast()
    for other in (b, c):
        g, f = other.get(blurred=True), other.get_fast()
        for k in ga:
            assert np.array_equal(ga[k], g[k]), k
        for k in fa:
            assert np.array_equal(fa[k], f[k]), k
    for x in (a, b, c, im, u):
        x.close()


# ---- one full frame

def test_vga_frame_default_parameters(pattern):
    from hslam_amd.extract import FeatureExtractor
    img = np.rint(cases.vga_image()).astype(np.uint8)
    want = fr.extract_fast(img, pattern)
    assert len(want["corner_xy"]) > 3000 and len(want["xy"]) > 1000 and want["ssc"]["exit"] == "found"
    e = FeatureExtractor(640, 480, 6000, pattern)
    n = e.extract_fast(img)
    first = (check_all(e, want, n), e.get_fast())
    assert e.last_stats() > 0
    assert e.extract_fast(img) == n                     # run to run
    second = (e.get(blurred=True), e.get_fast())
    for a, b in zip(first, second):
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    e.close()


# ---- lifetime

def test_create_fast_extract_destroy_returns_every_allocation(pattern):
    from hslam_amd._lib import load
    from hslam_amd.extract import FeatureExtractor
    lib = load()
    lib.hs_debug_live_allocations.argtypes, lib.hs_debug_live_allocations.restype = [], C.c_longlong
    gc.collect()
    start = lib.hs_debug_live_allocations()
    e = FeatureExtractor(W, H, 500, pattern)
    created = lib.hs_debug_live_allocations()
    assert created > start
    e.extract(np.zeros((H, W), np.float32), image("random"))
    assert lib.hs_debug_live_allocations() == created   # an extractor that never detects pays nothing
    e.extract_fast(image("random"))
    detecting = lib.hs_debug_live_allocations()
    assert detecting > created
    e.extract_fast(image("grey3"))
    assert lib.hs_debug_live_allocations() == detecting
    e.close()
    assert lib.hs_debug_live_allocations() == start
