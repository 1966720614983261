"""The undistortion kernel (hs_k_undistort) and its chaining into the tracker and the tracer, bit for bit against
tests/undist_ref.py fed the library's own table (Undistorter.remap()): the kernel's arithmetic is float32 in a fixed
order with every operation exactly rounded, so the bar is array_equal everywhere."""
import numpy as np
import pytest

import undist_ref
from undist_cases import CASES, gamma_G, lib_calib, random_vignette

pytestmark = pytest.mark.gpu


def _frame(name, seed=11):
    c = CASES[name]
    return np.random.default_rng(seed).integers(0, 256, size=(c["h_in"], c["w_in"]), dtype=np.uint8)


def _check(u, raw, G=None, vig=None, passthrough=False):
    """Sets the photometric tables, runs the device and the reference, compares fImg and img8."""
    u.set_photometric(G, vig)
    f, b = u.undistort(raw)
    rx, ry = u.remap()
    if G is None and vig is None:
        Binv = B = vinv = None
    else:
        Binv, B, vinv = undist_ref.make_photometric(G, vig)
        if G is None:
            Binv = None
    fr, br = undist_ref.undistort(raw, rx, ry, Binv, B, vinv, passthrough=passthrough)
    assert np.array_equal(f, fr)
    assert np.array_equal(b, br)
    return f


@pytest.fixture(scope="module")
def small():
    from hslam_amd.undistort import Undistorter
    u = Undistorter(lib_calib("small_usek"))
    yield u
    u.close()


@pytest.mark.parametrize("mode", ["none", "gamma", "vignette", "both"])
def test_small_usek_modes(small, mode):
    c = CASES["small_usek"]
    raw = _frame("small_usek")
    G = gamma_G() if mode in ("gamma", "both") else None
    vig = random_vignette((c["h_in"], c["w_in"])) if mode in ("vignette", "both") else None
    f = _check(small, raw, G, vig)
    rx, _ = small.remap()
    assert np.all(f[rx == -1] == 0) and np.any(f != 0)


def test_odd_sizes_crop():
    from hslam_amd.undistort import Undistorter
    u = Undistorter(lib_calib("odd_crop"))
    rx, _ = u.remap()
    assert not np.any(rx == -1)   # crop: every output pixel has a source
    _check(u, _frame("odd_crop"), gamma_G(), random_vignette((67, 101)))
    _check(u, _frame("odd_crop", seed=12))
    u.close()


def test_passthrough():
    from hslam_amd.undistort import Undistorter
    u = Undistorter(lib_calib("none"))
    raw = _frame("none")
    f = _check(u, raw, passthrough=True)
    assert np.array_equal(f, raw.astype(np.float32))
    _check(u, raw, gamma_G(), random_vignette((48, 64)), passthrough=True)
    assert np.array_equal(u.K, np.array(CASES["none"]["K_in"], np.float32))
    u.close()


def test_set_remap_handmade_map():
    """A caller's own 8 x 8 map over a 16 x 16 frame: the half-even cases of x * 32, the (-1, -1) marker and
    coordinates whose taps leave the frame on each side."""
    from hslam_amd.undistort import Undistorter, make_calib
    u = Undistorter(make_calib("Pinhole", 16, 16, 8, 8, (10.0, 10.0, 7.5, 7.5), process="crop"))
    gx, gy = np.meshgrid(np.arange(8, dtype=np.float32), np.arange(8, dtype=np.float32))
    rx, ry = gx * 1.5 + 2.25, gy * 1.5 + 1.75
    rx[0, :4] = [3 + 1 / 64, 4 + 3 / 64, 5 + 1 / 64, 6 + 3 / 64]   # x * 32 = k + 0.5: to even, down then up
    ry[1, :4] = [3 + 1 / 64, 4 + 3 / 64, 5 + 1 / 64, 6 + 3 / 64]
    rx[2, 0], ry[2, 0] = -1, -1
    rx[2, 1] = 16 - 1 + 0.5     # right taps outside
    ry[2, 2] = 16 + 2           # wholly below
    rx[2, 3] = -0.4             # left taps outside
    rx[2, 4], ry[2, 4] = -0.4, 15.5
    rx[2, 5], ry[2, 5] = 20, 20
    raw = np.random.default_rng(5).integers(1, 256, size=(16, 16), dtype=np.uint8)
    cls = undist_ref.tap_classes(raw.shape, rx, ry)
    assert np.any(cls == 4) and np.any((cls > 0) & (cls < 4)) and np.any(cls == 0)
    u.set_remap(rx, ry)
    gx2, gy2 = u.remap()
    assert np.array_equal(gx2, rx) and np.array_equal(gy2, ry)
    f = _check(u, raw)
    assert f[2, 2] == 0 and f[2, 5] == 0
    _check(u, raw, gamma_G(), random_vignette((16, 16)))
    from hslam_amd._lib import HsError
    bad = rx.copy()
    bad[0, 0] = 40000.0
    with pytest.raises(HsError, match="32767"):
        u.set_remap(bad, ry)
    u.close()


def test_euroc_full_size():
    from hslam_amd.undistort import Undistorter
    c = CASES["euroc"]
    u = Undistorter(lib_calib("euroc"))
    raw = _frame("euroc")
    _check(u, raw)
    _check(u, raw, gamma_G(), random_vignette((c["h_in"], c["w_in"])))
    u.close()


@pytest.fixture(scope="module")
def chain():
    """A 352 x 264 raw frame, its undistorter (320 x 240 out) and the reference's fImg of it, computed once."""
    from hslam_amd.undistort import Undistorter
    c = CASES["chain"]
    u = Undistorter(lib_calib("chain"))
    u.set_photometric(gamma_G(), None)
    # a smooth textured frame, so that tracking residuals and traces are meaningful
    y, x = np.mgrid[0:c["h_in"], 0:c["w_in"]].astype(np.float64)
    img = 128 + 60 * np.sin(x / 9.0) * np.cos(y / 7.0) + 40 * np.sin((x + 2 * y) / 23.0)
    raw = np.clip(img + np.random.default_rng(2).normal(0, 2, img.shape), 0, 255).astype(np.uint8)
    rx, ry = u.remap()
    Binv, B, _ = undist_ref.make_photometric(gamma_G(), None)
    fimg, _ = undist_ref.undistort(raw, rx, ry, Binv, B, None)
    yield u, raw, fimg
    u.close()


def test_tracker_u8_frame_matches_raw_frame(chain):
    from hslam_amd.scene import make_track_scene
    from hslam_amd.track import CoarseTracker
    u, raw, fimg = chain
    s = make_track_scene(n_points=400, width=320, height=240, n_levels=4,
                         K=np.array([[128.0, 0, 159.5], [0, 127.2, 119.5], [0, 0, 1.0]]))
    a = CoarseTracker(s.width, s.height, s.K4, s.n_levels)
    b = CoarseTracker(s.width, s.height, s.K4, s.n_levels)
    for t in (a, b):
        t.setCoarseTrackingRef(s.ref_pyr, s.ref_exposure, s.ref_aff, s.pt_u, s.pt_v, s.pt_idepth, s.pt_hdi)
    a.setNewFrameRaw(fimg, s.new_exposure)
    b.setNewFrameU8(u, raw, s.new_exposure)
    for lvl in range(s.n_levels):
        ra, Ha, ba_, na = a.calcRes(lvl, s.T_true, s.aff_true, 20.0)
        rb, Hb, bb_, nb = b.calcRes(lvl, s.T_true, s.aff_true, 20.0)
        assert na == nb and np.array_equal(ra, rb), lvl
        assert np.array_equal(Ha, Hb) and np.array_equal(ba_, bb_), lvl
        # the frame is unrelated to the scene's reference: a cutoff no residual reaches keeps every point in the sums
        ra, Ha, _, na = a.calcRes(lvl, s.T_true, s.aff_true, 1e4)
        rb, Hb, _, nb = b.calcRes(lvl, s.T_true, s.aff_true, 1e4)
        assert na == nb and na > 0 and np.array_equal(ra, rb) and np.array_equal(Ha, Hb), lvl
    a.close()
    b.close()


def test_tracer_u8_frame_matches_raw_frame(chain):
    from hslam_amd.scene import make_trace_scene
    from hslam_amd.trace import ImmatureTracer
    u, raw, fimg = chain
    s = make_trace_scene(n_points=500, n_hosts=4, width=320, height=240, seed=9)
    a = ImmatureTracer(s.width, s.height, s.n_points)
    b = ImmatureTracer(s.width, s.height, s.n_points)
    for t in (a, b):
        for i, im in enumerate(s.host_imgs):
            t.set_host_image(i, im)
        t.add_points(s.pt_host, s.pt_u, s.pt_v)
    a.set_frame_raw(fimg)
    b.set_frame_u8(u, raw)
    assert np.array_equal(a.traceNewCoarse(s.KRKi, s.Kt, s.aff), b.traceNewCoarse(s.KRKi, s.Kt, s.aff))
    pa, pb = a.points(), b.points()
    for k in pa:
        assert np.array_equal(pa[k], pb[k], equal_nan=True), k
    a.close()
    b.close()


def test_size_mismatch_is_invalid(small):
    """An undistorter whose output is not the consumer's size: HS_ERR_INVALID before any device work."""
    from hslam_amd._lib import HsError
    from hslam_amd.trace import ImmatureTracer
    from hslam_amd.track import CoarseTracker
    raw = _frame("small_usek")
    t = CoarseTracker(320, 240, (128.0, 127.2, 159.5, 119.5), 4)
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        t.setNewFrameU8(small, raw, 1.0)
    t.close()
    tr = ImmatureTracer(320, 240, 16)
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        tr.set_frame_u8(small, raw)
    tr.close()
