"""The keypoint-flow kernels (include/hs_flow.h) against tests/flow_ref.py, and their chaining behind the extractor
and the undistorter.  The contract has no transcendental function and no order-dependent float sum (the window sums
are exact integers), so the bar is array_equal on xy, status and err: a mismatch is a bug on one of the two sides."""
import ctypes as C
import gc

import numpy as np
import pytest

import flow_cases as cases
import flow_ref as ref

pytestmark = pytest.mark.gpu


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def check_calc(got, want):
    assert same(got["status"], want["status"]), np.flatnonzero(got["status"] != want["status"])[:8]
    assert same(got["xy"], want["xy"]), np.flatnonzero((got["xy"] != want["xy"]).any(axis=1))[:8]
    assert same(got["err"], want["err"]), np.flatnonzero(got["err"] != want["err"])[:8]


@pytest.fixture(scope="module")
def flows():
    """one context per coverage size, capacity = that case's point count"""
    from hslam_amd.flow import KeypointFlow
    out = []
    for k, (w, h) in enumerate(cases.COVERAGE_SIZES):
        out.append(KeypointFlow(w, h, len(cases.coverage_inputs(k)[2])))
    yield out
    for f in out:
        f.close()


# ---- pyramid and derivative

@pytest.mark.parametrize("k", [0, 2, 3])     # 96 x 80, 61 x 61 (odd sizes), 30 x 30 (one level)
def test_pyramid_and_derivative_levels(flows, k):
    a, b, pts = cases.coverage_inputs(k)
    fl = flows[k]
    fl.calc(a, b, pts[:1])
    for which, img in enumerate((a, b)):
        levels = ref.pyramid(img)
        assert fl.last_stats()[2] == len(levels) == ref.n_levels(*cases.COVERAGE_SIZES[k])
        for l, want in enumerate(levels):
            got_img, got_d = fl.pyramid(which, l)
            assert same(got_img, want), (which, l)
            assert same(got_d, ref.scharr(want)), (which, l)
    from hslam_amd._lib import HsError
    with pytest.raises(HsError, match=r"\(-1\).*level"):
        fl.pyramid(0, len(levels))
    with pytest.raises(HsError, match=r"\(-1\)"):
        fl.pyramid(2, 0)


# ---- the tracker against the reference

@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("k", range(len(cases.COVERAGE_SIZES)))
def test_calc_coverage_cases(flows, k, with_init):
    a, b, pts, init, want = cases.coverage_case(k, with_init)
    got = flows[k].calc(a, b, pts, init)
    check_calc(got, want)
    assert flows[k].last_stats()[1] == int(want["iters"].sum())
    assert 0 < int(want["status"].sum()) < len(pts)
    # two identical calls give identical results
    again = flows[k].calc(a, b, pts, init)
    for key in got:
        assert same(got[key], again[key]), key


def test_calc_shift_case_recovers_the_shift(flows):
    a, b, pts, shift, want = cases.shift_case(0)
    got = flows[0].calc(a, b, pts)
    check_calc(got, want)
    assert np.all(got["status"] == 1) and np.abs(got["xy"] - pts - shift).max() < 0.1


def test_non_finite_and_huge_coordinates(flows):
    a, b, pts = cases.coverage_inputs(0)
    w, h = cases.COVERAGE_SIZES[0]
    weird = np.array([[np.nan, 10], [10, np.nan], [np.inf, 10], [10, -np.inf], [1e30, 10], [10, -1e30],
                      [np.nan, np.nan], [-np.inf, np.inf], [3e38, 3e38]], np.float32)
    ok = np.tile(np.array([[w / 2 + 20.25, h / 2 - 25.5]], np.float32), (len(weird), 1))
    fl = flows[0]
    # in prev (no guess): status 0, err 0, the output is the input
    got = fl.calc(a, b, weird)
    check_calc(got, ref.calc(a, b, weird))
    assert not got["status"].any() and not got["err"].any()
    assert same(got["xy"], weird)
    # in the guess, the previous point being a good one
    got = fl.calc(a, b, ok, weird)
    check_calc(got, ref.calc(a, b, ok, weird))
    assert not got["status"].any() and not got["err"].any()
    assert same(got["xy"], weird)
    # in prev with a good guess
    got = fl.calc(a, b, weird, ok)
    check_calc(got, ref.calc(a, b, weird, ok))
    assert not got["status"].any() and not got["err"].any()
    assert same(got["xy"], ok)
    # and the context still tracks
    check_calc(fl.calc(a, b, pts[:5]), ref.calc(a, b, pts[:5]))


def test_point_counts_and_capacity(flows):
    from hslam_amd._lib import HsError
    a, b, pts, _, want = cases.coverage_case(1)
    fl = flows[1]
    cap = fl.capacity
    assert cap == len(pts)
    got = fl.calc(a, b, pts[:0])
    assert got["xy"].shape == (0, 2) and fl.last_stats()[1] == 0
    got = fl.calc(a, b, pts[:1])
    assert same(got["xy"], want["xy"][:1]) and same(got["err"], want["err"][:1])
    check_calc(fl.calc(a, b, pts), want)                        # n == capacity
    # the tracked state: n = 0 is legal, capacity + 1 is refused and leaves the prior result intact
    assert fl.set_first(a, pts[:0]) == 0
    assert fl.track(b, 7) == 0
    assert fl.get()["xy"].shape == (0, 2)
    fl.set_first(a, pts)
    n_good = fl.track(b, 7)
    before = fl.get()
    more = np.concatenate([pts, pts[:1]])
    with pytest.raises(HsError, match=r"\(-1\).*capacity"):
        fl.set_first(a, more)
    with pytest.raises(HsError, match=r"\(-1\).*capacity"):
        fl.calc(a, b, more)
    after = fl.get()
    for key in before:
        assert same(before[key], after[key]), key
    assert n_good == int(after["good"].sum())
    check_calc(after, want)                                     # a first track equals a calc without a guess


# ---- FindMatches' bookkeeping

def test_three_frame_chain():
    from hslam_amd._lib import HsError
    from hslam_amd.flow import KeypointFlow
    frames, pts, steps = cases.chain_case()
    fl = KeypointFlow(96, 80, len(pts) + 3)
    with pytest.raises(HsError, match=r"\(-5\)"):
        fl.track(frames[1], 7)                                  # before a first frame
    with pytest.raises(HsError, match=r"\(-5\)"):
        fl.mean_flow()
    assert fl.set_first(frames[0], pts) == len(pts)
    g = fl.get()
    assert same(g["first_xy"], pts) and same(g["prev_xy"], pts) and same(g["xy"], pts)
    assert not g["status"].any() and not g["good"].any() and not g["err"].any()
    with pytest.raises(HsError, match=r"\(-5\)"):
        fl.mean_flow()                                          # no track yet
    for img, want in zip(frames[1:], steps):
        n_good = fl.track(img, 7)
        g = fl.get()
        assert same(g["first_xy"], pts)
        assert same(g["prev_xy"], want["prev_xy"])
        check_calc(g, want)
        assert same(g["good"], want["good"])
        assert n_good == want["n_good"] == int(g["good"].sum())
        assert 0 < n_good < len(pts)                            # the out-of-image points fail
        assert fl.last_stats()[1] == want["iters"]
        m = fl.mean_flow()
        assert m == want["mean_flow"], (m, want["mean_flow"])
        # the quirk shows: a float sum of the same norms gives another mean
        d = (g["prev_xy"] - g["xy"])[g["good"] != 0].astype(np.float64)
        assert abs(float(m) - np.hypot(d[:, 0], d[:, 1]).mean()) > 0.25
    # failed points keep moving with their outputs: the second call's previous points are the first call's outputs
    assert same(steps[1]["prev_xy"], steps[0]["xy"])
    # the pyramids of the last track: previous = frame 1, next = frame 2
    assert same(fl.pyramid(0, 1)[0], ref.pyramid(frames[1])[1])
    assert same(fl.pyramid(1, 2)[0], ref.pyramid(frames[2])[2])
    fl.close()


# ---- behind the extractor and the undistorter (101 x 67, the extractor tests' size)

def test_extractor_hand_off():
    import extract_cases as xc
    from hslam_amd.extract import FeatureExtractor
    from hslam_amd.flow import KeypointFlow
    W, H = xc.W, xc.H
    img0, img1 = cases.image_pair(W, H, (1.25, -0.75), seed=60)
    m = xc.sparse_map(W, H, 7)
    ex = FeatureExtractor(W, H, 4000, xc.random_pattern())
    a, b = KeypointFlow(W, H, 4000), KeypointFlow(W, H, 4000)
    n = ex.extract(m, img0)
    keys = ex.get()["xy"]
    assert n == len(keys) > 50
    assert a.set_first_extracted(ex) == n
    b.set_first(img0, keys)
    ga, gb = a.get(), b.get()
    for key in ga:
        assert same(ga[key], gb[key]), key
    ex.extract(np.zeros((H, W), np.float32), img1)               # the new frame's cvImgL, no keys needed
    na, nb = a.track_extracted(ex, 7), b.track(img1, 7)
    ga, gb = a.get(), b.get()
    for key in ga:
        assert same(ga[key], gb[key]), key
    assert na == nb > n // 2
    check_calc(ga, ref.calc(img0, img1, keys, keys))
    assert same(a.pyramid(1, 0)[0], img1) and same(a.pyramid(0, 0)[0], img0)
    for f in (a, b):
        f.close()
    ex.close()


def test_undistorter_hand_off():
    from hslam_amd.flow import KeypointFlow
    from hslam_amd.undistort import Undistorter, make_calib
    from undist_cases import EUROC_DIST, gamma_G
    W, H = 101, 67
    u = Undistorter(make_calib("RadTan", 118, 80, W, H, (75.0, 74.0, 58.5, 39.5), EUROC_DIST, "useK",
                               (0.55, 0.73, 0.5, 0.5)))
    u.set_photometric(gamma_G(), None)
    f0 = cases.field(118, 80, seed=61)
    raw0 = cases.crop8(f0)
    raw1 = cases.crop8(np.clip(cases.ndimage.shift(f0, (0.5, 1.5), order=3, mode="nearest"), 0, 255))
    _, img0 = u.undistort(raw0)
    _, img1 = u.undistort(raw1)
    pts = cases.interior_points(W, H, 150, seed=62)
    a, b = KeypointFlow(W, H, 150), KeypointFlow(W, H, 150)
    for f in (a, b):
        f.set_first(img0, pts)
    na, nb = a.track_u8(u, raw1, 7), b.track(img1, 7)
    ga, gb = a.get(), b.get()
    for key in ga:
        assert same(ga[key], gb[key]), key
    assert na == nb > 75
    assert same(a.pyramid(1, 0)[0], img1)
    for f in (a, b):
        f.close()
    u.close()


def test_mismatches_and_null_arguments(flows):
    import extract_cases as xc
    from hslam_amd._lib import HsError, load, ptr
    from hslam_amd.extract import FeatureExtractor
    from hslam_amd.flow import KeypointFlow
    from hslam_amd.undistort import Undistorter
    from undist_cases import lib_calib
    lib = load()
    a, b, pts = cases.coverage_inputs(1)                         # 64 x 48
    fl = flows[1]
    fl.set_first(a, pts)
    ex = FeatureExtractor(xc.W, xc.H, 100, xc.random_pattern())  # 101 x 67
    with pytest.raises(HsError, match=r"\(-5\).*extract"):
        fl.track_extracted(ex, 7)                                # the extractor holds no image yet
    ex.extract(np.zeros((xc.H, xc.W), np.float32), xc.random_image())
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        fl.track_extracted(ex, 7)
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        fl.set_first_extracted(ex)
    ex.close()
    u = Undistorter(lib_calib("small_usek"))                     # 64 x 48 out: fits flows[1], not flows[0]
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        flows[0].track_u8(u, np.zeros((u.h_in, u.w_in), np.uint8), 7)
    u.close()
    n = C.c_int(-7)
    assert lib.hs_flow_track(fl.h, None, 7.0, C.byref(n)) == -1
    assert lib.hs_flow_set_first(fl.h, None, 1, ptr(pts)) == -1
    assert lib.hs_flow_set_first(fl.h, ptr(a), 1, None) == -1
    assert lib.hs_flow_calc(fl.h, ptr(a), None, 1, ptr(pts), None, None, None, None) == -1
    assert lib.hs_flow_calc(fl.h, ptr(a), ptr(b), 1, None, None, None, None, None) == -1
    assert lib.hs_flow_track_extracted(fl.h, None, 7.0, C.byref(n)) == -1
    assert lib.hs_flow_track_u8(fl.h, None, ptr(a), 7.0, C.byref(n)) == -1
    assert lib.hs_flow_mean_flow(fl.h, None) == -1
    assert n.value == -7
    assert lib.hs_flow_track(fl.h, ptr(b), 7.0, None) == 0       # the count is optional
    with pytest.raises(ValueError):
        fl.track(b[:-1], 7)
    # another device: refused where there is one, an invalid id where there is not
    with pytest.raises(HsError, match=r"\(-1\).*device"):
        KeypointFlow(64, 48, 10, device=4096)
    with pytest.raises(HsError, match=r"\(-1\).*16"):
        KeypointFlow(15, 48, 10)
    try:
        far = FeatureExtractor(64, 48, 100, xc.random_pattern(), device=1)
    except HsError as err:
        assert "(-1)" in str(err) and "device" in str(err)
    else:
        far.extract(np.zeros((48, 64), np.float32), a)
        with pytest.raises(HsError, match=r"\(-1\).*device"):
            fl.track_extracted(far, 7)
        far.close()


# ---- lifetime

def test_create_and_failed_create_return_every_allocation():
    from hslam_amd._lib import load
    lib = load()
    lib.hs_debug_live_allocations.argtypes, lib.hs_debug_live_allocations.restype = [], C.c_longlong
    gc.collect()
    start = lib.hs_debug_live_allocations()
    a, b, pts = cases.coverage_inputs(1)
    xy = np.zeros((len(pts), 2), np.float32)
    for _ in range(3):
        h = C.c_void_p()
        assert lib.hs_flow_create(C.byref(h), 0, 64, 48, len(pts)) == 0
        assert lib.hs_debug_live_allocations() > start
        assert lib.hs_flow_calc(h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), len(pts),
                                pts.ctypes.data_as(C.c_void_p), None, xy.ctypes.data_as(C.c_void_p), None, None) == 0
        lib.hs_flow_destroy(h)
        assert lib.hs_debug_live_allocations() == start
    h = C.c_void_p(1)
    assert lib.hs_flow_create(C.byref(h), 4096, 64, 48, 10) == -1     # no such device
    assert not h.value and lib.hs_debug_live_allocations() == start
    h = C.c_void_p(1)
    assert lib.hs_flow_create(C.byref(h), 0, 64, 15, 10) == -1        # refused before any allocation
    assert not h.value and lib.hs_debug_live_allocations() == start
