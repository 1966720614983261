"""The extraction kernels (include/hs_extract.h) against tests/extract_ref.py, and their chaining behind the selector
and the undistorter and in front of the tracer.  Keys, the blur and the angles are integer or exactly rounded float32
arithmetic in a fixed order: the bar is array_equal.  The descriptor goes through cos / sin in double, where two math
libraries may differ in the last place: every bit the reference does not flag ambiguous (a tap coordinate within 1e-4
of a rounding tie) must match, flagged bits may differ, and the flagged share is asserted <= 0.5 % wherever the
allowance is used, so it cannot hide a broken kernel."""
import numpy as np
import pytest

import extract_cases as cases
import extract_ref as ref

pytestmark = pytest.mark.gpu

W, H = cases.W, cases.H


@pytest.fixture(scope="module")
def pattern():
    return cases.random_pattern()


@pytest.fixture(scope="module")
def ex(pattern):
    """An extractor at 101 x 67 whose capacity is the whole interior."""
    from hslam_amd.extract import FeatureExtractor
    e = FeatureExtractor(W, H, (W - 38) * (H - 38), pattern)
    yield e
    e.close()


def check_against(got, want):
    """got: FeatureExtractor.get(blurred=True); want: extract_ref.extract of the same inputs."""
    assert np.array_equal(got["blurred"], want["blurred"])
    assert np.array_equal(got["xy"], want["xy"])
    assert np.array_equal(got["angle"], want["angle"])
    share = cases.ambiguous_share(want)
    assert share <= cases.MAX_AMBIGUOUS, share
    differ = ref.unpack_bits(got["desc"]) != ref.unpack_bits(want["desc"])
    assert not np.any(differ & ~want["ambiguous"]), int(np.sum(differ & ~want["ambiguous"]))


# ---- blur

@pytest.mark.parametrize("w,h", [(101, 67), (96, 64), (39, 39)])
def test_blur_random(pattern, w, h):
    from hslam_amd.extract import FeatureExtractor
    e = FeatureExtractor(w, h, 16, pattern)
    img = cases.random_image(w, h, seed=w)
    assert e.extract(np.zeros((h, w), np.float32), img) == 0
    assert np.array_equal(e.get(blurred=True)["blurred"], ref.blur(img))
    e.close()


def test_blur_saturated(ex):
    img = np.full((H, W), 255, np.uint8)
    ex.extract(np.zeros((H, W), np.float32), img)
    assert np.array_equal(ex.get(blurred=True)["blurred"], img)


# ---- keys

def handmade_map():
    m = np.zeros((H, W), np.float32)
    m[19, 19], m[19, W - 20], m[H - 20, 19], m[H - 20, W - 20] = 1, 2, 4, -1.5   # the interior's corners
    m[18, 40] = m[H - 19, 40] = m[30, 18] = m[30, W - 19] = 1                      # just outside each side
    m[0, 0] = m[H - 1, W - 1] = m[18, 18] = m[H - 19, W - 19] = 4
    m[33, :] = 2                                                                   # one full row
    m[25, 20], m[25, 21], m[40, 80] = 1, 4, 2
    return m


def test_keys_handmade_map(ex):
    m = handmade_map()
    img = cases.random_image()
    n = ex.extract(m, img)
    want = ref.keys(m)
    assert n == len(want) == 4 + (W - 38) + 3
    got = ex.get()
    assert np.array_equal(got["xy"], want)
    assert got["xy"][0].tolist() == [19, 19] and got["xy"][-1].tolist() == [W - 20, H - 20]
    # a second, identical call gives the identical result
    assert ex.extract(m, img) == n
    again = ex.get()
    for k in got:
        assert np.array_equal(got[k], again[k]), k


def test_keys_empty_map_then_fewer_keys(ex):
    img = cases.random_image()
    assert ex.extract(handmade_map(), img) > 3
    assert ex.extract(np.zeros((H, W), np.float32), img) == 0
    got = ex.get(blurred=True)
    assert got["xy"].shape == (0, 2) and got["angle"].shape == (0,) and got["desc"].shape == (0, 32)
    assert np.array_equal(got["blurred"], ref.blur(img))
    m = np.zeros((H, W), np.float32)
    m[30, 30] = m[31, 29] = 1
    assert ex.extract(m, img) == 2
    assert ex.get()["xy"].tolist() == [[30, 30], [29, 31]]


def test_keys_single_candidate_pixel(pattern):
    from hslam_amd.extract import FeatureExtractor
    e = FeatureExtractor(39, 39, 1, pattern)
    img = cases.random_image(39, 39, seed=5)
    m = np.ones((39, 39), np.float32)
    assert e.extract(m, img) == 1
    check_against(e.get(blurred=True), ref.extract(m, img, pattern))
    assert e.get()["xy"].tolist() == [[19, 19]]
    e.close()


def test_capacity_exact_and_one_less(ex, pattern):
    from hslam_amd.extract import ExtractOverflow, FeatureExtractor
    interior = (W - 38) * (H - 38)
    ones = np.ones((H, W), np.float32)
    img = cases.random_image()
    assert ex.extract(ones, img) == interior          # capacity == the interior's size
    assert np.array_equal(ex.get()["xy"], ref.keys(ones))
    small = FeatureExtractor(W, H, interior - 1, pattern)
    m = np.zeros((H, W), np.float32)
    m[30, 30] = m[31, 29] = 1
    img2 = cases.random_image(seed=8)
    assert small.extract(m, img2) == 2
    before = small.get(blurred=True)
    with pytest.raises(ExtractOverflow, match=r"\(-1\)") as ei:
        small.extract(ones, img)
    assert ei.value.needed == interior
    after = small.get(blurred=True)                    # nothing truncated, the previous result still readable
    assert after["xy"].tolist() == [[30, 30], [29, 31]]
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert small.extract(m, img2) == 2                 # and the extractor still works
    small.close()


# ---- angles and descriptors

def test_random_image_angles_and_descriptors(ex):
    m, img, pat, want = cases.descriptor_case()
    assert ex.extract(m, img) == len(want["xy"]) > 300
    got = ex.get(blurred=True)
    check_against(got, want)
    assert len(np.unique(got["desc"], axis=0)) > 0.9 * len(got["desc"])   # not a constant


def test_uniform_image_angle_zero(ex, pattern):
    m = cases.sparse_map(W, H, 7)
    img = np.full((H, W), 90, np.uint8)
    assert ex.extract(m, img) > 50
    got = ex.get(blurred=True)
    assert np.all(got["angle"] == 0)
    assert np.all(got["desc"] == 0)   # no pixel is darker than another
    check_against(got, ref.extract(m, img, pattern))


@pytest.mark.parametrize("sx,sy,lo,hi", [(1, 1, 0, 90), (-1, 1, 90, 180), (-1, -1, 180, 270), (1, -1, 270, 360)])
def test_ramp_image_quadrants(ex, pattern, sx, sy, lo, hi):
    m = cases.sparse_map(W, H, 7)
    img = cases.ramp_image(sx, sy)
    assert ex.extract(m, img) > 50
    got = ex.get(blurred=True)
    assert np.all((got["angle"] > lo) & (got["angle"] < hi))
    check_against(got, ref.extract(m, img, pattern))


# ---- behind the selector and the undistorter

def test_selector_chain_small(pattern):
    from hslam_amd.extract import FeatureExtractor
    from hslam_amd.scene import make_select_frames
    from hslam_amd.select import PixelSelector
    w, h = 160, 96
    frames = make_select_frames(2, width=w, height=h, contrast_ramp=True, seed=3)
    sel = PixelSelector(w, h)
    a = FeatureExtractor(w, h, 4000, pattern)
    b = FeatureExtractor(w, h, 4000, pattern)
    for fid, f in enumerate(frames):
        img = np.rint(f).astype(np.uint8)
        m, _ = sel.makeMapsRaw(f, fid, 600)
        na = a.extract_selected(sel, img)
        nb = b.extract(m, img)
        assert na == nb == len(ref.keys(m)) > 50
        ga, gb = a.get(blurred=True), b.get(blurred=True)
        for k in ga:
            assert np.array_equal(ga[k], gb[k]), (fid, k)
    assert a.last_stats() > 0
    a.close()
    b.close()


def test_selector_chain_vga_against_reference(pattern):
    from hslam_amd.extract import FeatureExtractor
    from hslam_amd.select import PixelSelector
    f = cases.vga_image()
    img = np.rint(f).astype(np.uint8)
    sel = PixelSelector(640, 480)
    e = FeatureExtractor(640, 480, 6000, pattern)
    m, _ = sel.makeMapsRaw(f, 0, 2000)
    n = e.extract_selected(sel, img)
    assert n > 500
    check_against(e.get(blurred=True), ref.extract(m, img, pattern))
    e.close()


def test_undistorter_chain(pattern):
    from hslam_amd.extract import FeatureExtractor
    from hslam_amd.scene import make_select_frames
    from hslam_amd.select import PixelSelector
    from hslam_amd.undistort import Undistorter, make_calib
    from undist_cases import EUROC_DIST, gamma_G
    w, h = 160, 96
    u = Undistorter(make_calib("RadTan", 176, 112, w, h, (110.0, 109.0, 87.5, 55.5), EUROC_DIST, "useK",
                               (0.55, 0.73, 0.5, 0.5)))
    u.set_photometric(gamma_G(), None)
    raw = np.random.default_rng(6).integers(0, 256, size=(112, 176), dtype=np.uint8)
    sel = PixelSelector(w, h)
    m, _ = sel.makeMapsRaw(make_select_frames(1, width=w, height=h, contrast_ramp=True, seed=3)[0], 0, 600)
    a = FeatureExtractor(w, h, 4000, pattern)
    b = FeatureExtractor(w, h, 4000, pattern)
    na = a.extract_u8(sel, u, raw)
    _, img8 = u.undistort(raw)
    nb = b.extract(m, img8)
    assert na == nb > 50
    ga, gb = a.get(blurred=True), b.get(blurred=True)
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    assert np.array_equal(ga["blurred"], ref.blur(img8))
    a.close()
    b.close()
    u.close()


# ---- in front of the tracer

def test_tracer_add_keys_matches_add_points(ex):
    from hslam_amd._lib import HsError
    from hslam_amd.trace import ImmatureTracer
    m, img, _, want = cases.descriptor_case()
    n = ex.extract(m, img)
    xy = ex.get()["xy"]
    rng = np.random.default_rng(12)
    host = [rng.uniform(0, 255, size=(H, W, 3)).astype(np.float32) for _ in range(2)]
    a = ImmatureTracer(W, H, 2 * n + 5)
    b = ImmatureTracer(W, H, 2 * n + 5)
    for t in (a, b):
        t.set_host_image(0, host[0])
        t.set_host_image(2, host[1])
    # behind existing points, then a second batch on another slot
    a.add_points([0, 0], [30.5, 41.0], [22.0, 33.25])
    b.add_points([0, 0], [30.5, 41.0], [22.0, 33.25])
    assert a.add_keys(ex, 0) == n
    assert a.add_keys(ex, 2) == n
    b.add_points(np.zeros(n, np.int32), xy[:, 0], xy[:, 1])
    b.add_points(np.full(n, 2, np.int32), xy[:, 0], xy[:, 1])
    assert a.n == b.n == 2 * n + 2
    pa, pb = a.points(), b.points()
    for k in pa:
        assert pa[k].shape == pb[k].shape and np.array_equal(pa[k], pb[k], equal_nan=True), k
    assert np.any(pa["color"] != 0)
    # capacity: 2n + 5 holds 2n + 2; another n do not fit, and nothing is added
    with pytest.raises(HsError, match=r"\(-1\).*capacity"):
        a.add_keys(ex, 0)
    assert a.n == 2 * n + 2
    with pytest.raises(HsError, match=r"\(-1\).*slot"):
        a.add_keys(ex, 1)          # a slot without an image
    with pytest.raises(HsError, match=r"\(-1\).*slot"):
        a.add_keys(ex, 99)
    # the tracer goes on as after add_points: both trace the same
    for t in (a, b):
        t.set_frame(host[1])
    eye = np.tile(np.eye(3, dtype=np.float32).ravel(), (3, 1))
    Kt = np.tile(np.array([0.8, 0.1, 0.0], np.float32), (3, 1))
    aff = np.tile(np.array([1.0, 0.0], np.float32), (3, 1))
    assert np.array_equal(a.traceNewCoarse(eye, Kt, aff), b.traceNewCoarse(eye, Kt, aff))
    a.close()
    b.close()
    c = ImmatureTracer(W + 1, H, 10)
    c.set_host_image(0, np.zeros((H, W + 1, 3), np.float32))
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        c.add_keys(ex, 0)
    c.close()


# ---- bad arguments

def test_bad_arguments(ex, pattern):
    import ctypes as C
    from hslam_amd._lib import HsError, load, ptr
    from hslam_amd.extract import FeatureExtractor
    from hslam_amd.select import PixelSelector
    from hslam_amd.undistort import Undistorter
    from undist_cases import lib_calib
    lib = load()
    n = C.c_int(-7)
    m = np.zeros((H, W), np.float32)
    img = cases.random_image()
    assert lib.hs_extractor_extract(ex.h, None, ptr(img), C.byref(n)) == -1
    assert lib.hs_extractor_extract(ex.h, ptr(m), None, C.byref(n)) == -1
    assert lib.hs_extractor_extract_selected(ex.h, None, ptr(img), C.byref(n)) == -1
    assert lib.hs_extractor_extract(ex.h, ptr(m), ptr(img), None) == 0        # the count is optional
    with pytest.raises(ValueError):
        ex.extract(m, img[:-1])
    w, h = 160, 96
    e = FeatureExtractor(w, h, 4000, pattern)
    img = cases.random_image(w, h, seed=13)
    sel = PixelSelector(w, h)
    assert lib.hs_extractor_extract_selected(e.h, sel.h, None, C.byref(n)) == -1
    assert lib.hs_extractor_extract_u8(e.h, sel.h, None, ptr(img), C.byref(n)) == -1
    with pytest.raises(HsError, match=r"\(-5\).*no map"):
        e.extract_selected(sel, img)                                           # before any makeMaps
    other = PixelSelector(128, h)
    other.makeMapsRaw(cases.random_image(128, h, seed=14).astype(np.float32), 0, 100.0)
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        e.extract_selected(other, img)
    sel.makeMapsRaw(img.astype(np.float32), 0, 100.0)
    assert e.extract_selected(sel, img) > 0                                    # and now it runs
    u = Undistorter(lib_calib("small_usek"))                                   # 64 x 48 out
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        e.extract_u8(sel, u, np.zeros((u.h_in, u.w_in), np.uint8))
    u.close()
    # another device: refused where there is one, an invalid id where there is not
    try:
        far = PixelSelector(w, h, device=1)
    except HsError as err:
        assert "(-1)" in str(err) and "device" in str(err)
    else:
        far.makeMapsRaw(img.astype(np.float32), 0, 100.0)
        with pytest.raises(HsError, match=r"\(-1\).*device"):
            e.extract_selected(far, img)
    with pytest.raises(HsError, match=r"\(-1\).*device"):
        FeatureExtractor(w, h, 10, pattern, device=4096)
    e.close()
