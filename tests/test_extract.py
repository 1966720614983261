"""The extraction contract's reference (tests/extract_ref.py) against the rules of include/hs_extract.h, the argument
checks of hs_extractor_create that come before any device call, and the condition the device tests' descriptor
allowance rests on.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import extract_cases as cases
import extract_ref as ref


def test_blur_weights():
    w = ref.blur_weights()
    assert w.tolist() == [18, 34, 48, 56, 48, 34, 18]
    assert w.sum() == 256


def test_blur_constant_and_impulse():
    for v in (0, 1, 77, 255):
        img = np.full((41, 45), v, np.uint8)
        assert np.array_equal(ref.blur(img), img)
    img = np.zeros((41, 45), np.uint8)
    img[20, 22] = 255
    w = ref.blur_weights()
    want = np.zeros((41, 45), np.int64)
    want[17:24, 19:26] = (np.outer(w, w) * 255 + 32768) >> 16
    assert np.array_equal(ref.blur(img), want.astype(np.uint8))


def test_blur_reflects_without_repeating_the_edge():
    """REFLECT_101: an impulse one pixel inside the left edge is counted twice at the edge column's tap pair."""
    img = np.zeros((39, 39), np.uint8)
    img[10, 1] = 255
    w = ref.blur_weights()
    out = ref.blur(img).astype(np.int64)
    # column 0 gathers source columns r(-3..3) = 3 2 1 0 1 2 3: the impulse at 1 under taps 2 and 4
    h0 = (w[2] + w[4]) * 255
    assert out[10, 0] == (w[3] * h0 + 32768) >> 16
    # column 1 gathers 2 1 0 1 2 3 4: taps 1 and 3
    assert out[10, 1] == (w[3] * (w[1] + w[3]) * 255 + 32768) >> 16


def test_umax_symmetric():
    um = ref.umax()
    assert um.tolist() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    # the disc is symmetric about its diagonal: (u, v) inside <=> (v, u) inside
    inside = np.array([[abs(u) <= um[abs(v)] for u in range(-15, 16)] for v in range(-15, 16)])
    assert np.array_equal(inside, inside.T)
    assert np.all(np.diff(um) <= 0)


def test_fast_atan2():
    f = ref.fast_atan2
    assert f(0, 1)[0] == 0 and f(0, -1)[0] == 180 and f(1, 0)[0] == 90 and f(-1, 0)[0] == 270
    assert f(0, 12345)[0] == 0 and f(-777, 0)[0] == 270
    assert f(0, 0)[0] == 0
    rng = np.random.default_rng(3)
    y = rng.integers(-2 ** 24 + 1, 2 ** 24, 20000).astype(np.float32)
    x = rng.integers(-2 ** 24 + 1, 2 ** 24, 20000).astype(np.float32)
    y[:2000] = rng.integers(-40, 41, 2000)   # small moments too
    x[:2000] = rng.integers(-40, 41, 2000)
    keep = (x != 0) | (y != 0)
    a = f(y, x)[keep].astype(np.float64)
    want = np.degrees(np.arctan2(y[keep].astype(np.float64), x[keep].astype(np.float64))) % 360.0
    d = np.abs(a - want)
    d = np.minimum(d, 360.0 - d)
    assert d.max() <= 0.3, d.max()   # the accuracy OpenCV documents for fastAtan2
    assert a.min() >= 0 and a.max() <= 360


def test_keys_raster_order_and_interior():
    m = np.zeros((cases.H, cases.W), np.float32)
    m[18, 30] = m[19, 18] = m[cases.H - 19, 30] = m[30, cases.W - 19] = 1   # just outside
    m[19, 19] = 1
    m[19, cases.W - 20] = 2
    m[40, 50] = -3
    m[cases.H - 20, 19] = 4
    assert ref.keys(m).tolist() == [[19, 19], [cases.W - 20, 19], [50, 40], [19, cases.H - 20]]


def test_descriptor_bits_by_hand():
    """Angle 0 (a uniform image): a = 1, b = 0, the taps are the pattern itself."""
    pat = cases.random_pattern()
    img = np.full((cases.H, cases.W), 90, np.uint8)
    xy = np.array([[40, 30]], np.float32)
    ang = ref.angles(img, xy)
    assert ang[0] == 0
    blurred = cases.random_image(seed=4)
    desc, amb = ref.descriptors(blurred, xy, ang, pat)
    assert not amb.any()
    bits = ref.unpack_bits(desc)[0]
    for i in range(256):
        (px, py), (qx, qy) = pat[i].astype(int)
        assert bits[i] == (blurred[30 + py, 40 + px] < blurred[30 + qy, 40 + qx]), i


def _create(w, h, cap, pattern):
    from hslam_amd import _lib
    lib = _lib.load()
    h_ = C.c_void_p()
    pat = np.ascontiguousarray(pattern, np.int8)
    rc = lib.hs_extractor_create(C.byref(h_), 0, w, h, cap, _lib.ptr(pat))
    if rc == 0:
        lib.hs_extractor_destroy(h_)
    return rc, lib.hs_last_error().decode()


def test_create_rejects_bad_arguments_before_the_device():
    good = cases.random_pattern().ravel()
    for k, v in ((0, 14), (1023, -14), (517, 127), (3, -128)):
        bad = good.copy()
        bad[k] = v
        rc, msg = _create(64, 64, 100, bad)
        assert rc == -1 and "13" in msg and str(k) in msg, (rc, msg)
    rc, msg = _create(38, 64, 100, good)
    assert rc == -1 and "39" in msg
    rc, msg = _create(64, 38, 100, good)
    assert rc == -1 and "39" in msg
    rc, msg = _create(64, 64, 0, good)
    assert rc == -1 and "capacity" in msg
    from hslam_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.hs_extractor_create(C.byref(h), 0, 64, 64, 10, None) == -1
    assert lib.hs_extractor_create(None, 0, 64, 64, 10, _lib.ptr(good)) == -1
    # null contexts never reach a device either
    n = C.c_int()
    assert lib.hs_extractor_extract(None, None, None, C.byref(n)) == -1
    assert lib.hs_extractor_get(None, C.byref(n), None, None, None, None) == -1
    assert lib.hs_tracer_add_keys(None, None, 0, C.byref(n)) == -1


def test_binding_checks_pattern_length():
    from hslam_amd._lib import HsError
    from hslam_amd.extract import FeatureExtractor
    with pytest.raises(HsError, match="256 x 2 x 2"):
        FeatureExtractor(64, 64, 10, np.zeros(1000, np.int8))


def test_ambiguous_share_of_the_device_tests_inputs():
    """The device tests let a descriptor bit differ where the reference flags it ambiguous.  That allowance is only
    sound while few bits are flagged: the cap holds for every input the device tests compare descriptors on."""
    pat = cases.random_pattern()
    shares = {"random": cases.ambiguous_share(cases.descriptor_case()[3])}
    for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1)):
        shares[f"ramp{sx}{sy}"] = cases.ambiguous_share(
            ref.extract(cases.sparse_map(cases.W, cases.H, 7), cases.ramp_image(sx, sy), pat))
    img = np.rint(cases.vga_image()).astype(np.uint8)
    shares["vga"] = cases.ambiguous_share(ref.extract(cases.sparse_map(640, 480, 151), img, pat))
    for k, s in shares.items():
        assert s <= cases.MAX_AMBIGUOUS, (k, s)
    # and the flag is not vacuous: 2000 random angles flag some bits, far fewer than the cap
    ang = np.random.default_rng(9).uniform(0, 360, 2000).astype(np.float32)
    amb = ref.ambiguous_bits(*ref.tap_offsets(ang, pat))
    assert 0 < amb.mean() <= cases.MAX_AMBIGUOUS
