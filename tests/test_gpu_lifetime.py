"""Every object behind the C ABI gives back exactly the device and pinned allocations it took: the process-wide count
of h-slam_amd/csrc/hs_host.h's pools (hs_debug_live_allocations) returns to its start after create, first use and
destroy, a regrow releases what it replaces, and the one-shot entry points leave nothing behind.  Equalities, at the
smallest sizes the creates accept; the C ABI is called directly so that no wrapper's finalizer moves the count."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, CAP = 64, 48, 64
K4 = (60.0, 60.0, 31.5, 23.5)


@pytest.fixture(scope="module")
def lib():
    from hslam_amd._lib import load
    lib = load()
    lib.hs_debug_live_allocations.argtypes, lib.hs_debug_live_allocations.restype = [], C.c_longlong
    gc.collect()  # wrappers other tests dropped free their objects now, not between two reads of the count
    return lib


def _ok(lib, rc):
    assert rc == 0, lib.hs_last_error().decode(errors="replace")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _triplets(w, h, seed=3):
    return np.random.default_rng(seed).random((h, w, 3), dtype=np.float32)


def _camera(w=W, h=H):
    from hslam_amd._lib import hs_camera
    return hs_camera(w, h, 2, 0, *K4)


def _ba(lib, points=None):
    """a BA context; points: the capacities of the window reserves made on it, in order"""
    from hslam_amd._lib import default_params
    p, h, cam = default_params(), C.c_void_p(), _camera()
    _ok(lib, lib.hs_create(C.byref(h), C.byref(p), 0))
    for n in points or ():
        _ok(lib, lib.hs_ba_reserve(h, C.byref(cam), n))
    return h


def _tracker(lib):
    from hslam_amd._lib import default_params
    p, h, k4 = default_params(), C.c_void_p(), np.array(K4, np.float32)
    _ok(lib, lib.hs_tracker_create(C.byref(h), C.byref(p), 0, W, H, 2, _p(k4)))
    pyr = [_triplets(W >> l, H >> l) for l in range(2)]  # set_ref allocates the reference points
    pp = (C.c_void_p * 2)(*[a.ctypes.data for a in pyr])
    aff = np.zeros(2, np.float64)
    u = np.array([10, 20, 30, 40, 50], np.float32)
    v = np.array([8, 16, 24, 32, 40], np.float32)
    idepth, hdi = np.full(5, 0.5, np.float32), np.full(5, 1.0, np.float32)
    _ok(lib, lib.hs_tracker_set_ref(h, C.cast(pp, C.c_void_p), 1.0, _p(aff), 5, _p(u), _p(v), _p(idepth), _p(hdi)))
    return h


def _tracer(lib):
    from hslam_amd._lib import default_params
    p, h = default_params(), C.c_void_p()
    _ok(lib, lib.hs_tracer_create(C.byref(h), C.byref(p), 0, W, H, CAP))
    img = _triplets(W, H)  # a host slot's image is allocated on its first upload
    _ok(lib, lib.hs_tracer_set_host_image(h, 0, _p(img)))
    host = np.zeros(4, np.int32)
    u, v = np.array([10, 20, 30, 40], np.float32), np.array([8, 16, 24, 32], np.float32)
    _ok(lib, lib.hs_tracer_add_points(h, 4, _p(host), _p(u), _p(v)))
    return h


def _selector(lib):
    from hslam_amd._lib import default_params
    p, h = default_params(), C.c_void_p()
    _ok(lib, lib.hs_selector_create(C.byref(h), C.byref(p), 0, W, H))
    return h


def _extractor(lib):
    h = C.c_void_p()
    pattern = np.random.default_rng(5).integers(-13, 14, size=1024).astype(np.int8)
    _ok(lib, lib.hs_extractor_create(C.byref(h), 0, W, H, CAP, _p(pattern)))
    return h


def _undistorter(lib):
    from undist_cases import lib_calib
    h, calib = C.c_void_p(), lib_calib("small_usek")  # 96 x 64 -> 64 x 48
    _ok(lib, lib.hs_undistorter_create(C.byref(h), 0, C.byref(calib)))
    return h


def _refiner(lib, n=5):
    h, k4 = C.c_void_p(), np.array(K4, np.float64)
    _ok(lib, lib.hs_refiner_create(C.byref(h), 0, W, H, _p(k4)))
    _refiner_points(lib, h, n)
    return h


def _refiner_points(lib, h, n):
    u, v = np.linspace(4, W - 5, n).astype(np.float32), np.linspace(4, H - 5, n).astype(np.float32)
    tri, z = np.ones(n, np.uint8), np.full(n, 2.0, np.float32)
    _ok(lib, lib.hs_refiner_set_points(h, n, _p(u), _p(v), _p(tri), _p(z)))


OBJECTS = {
    "ba": (lambda lib: _ba(lib, [1]), "hs_destroy"),
    "tracker": (_tracker, "hs_tracker_destroy"),
    "tracer": (_tracer, "hs_tracer_destroy"),
    "selector": (_selector, "hs_selector_destroy"),
    "extractor": (_extractor, "hs_extractor_destroy"),
    "undistorter": (_undistorter, "hs_undistorter_destroy"),
    "refiner": (_refiner, "hs_refiner_destroy"),
}


@pytest.mark.parametrize("name", list(OBJECTS))
def test_create_use_destroy_returns_every_allocation(lib, name):
    make, destroy = OBJECTS[name]
    start = lib.hs_debug_live_allocations()
    for _ in range(3):  # a double free or a stale record of round one would show in round two
        h = make(lib)
        assert lib.hs_debug_live_allocations() > start
        getattr(lib, destroy)(h)
        assert lib.hs_debug_live_allocations() == start


def test_ba_regrow_releases_what_it_replaces(lib):
    start = lib.hs_debug_live_allocations()
    fresh = _ba(lib, [CAP])
    n_fresh = lib.hs_debug_live_allocations() - start
    lib.hs_destroy(fresh)
    assert lib.hs_debug_live_allocations() == start
    grown = _ba(lib, [1, CAP])  # the second reserve needs more points: every capacity buffer is replaced
    assert lib.hs_debug_live_allocations() - start == n_fresh
    lib.hs_destroy(grown)
    assert lib.hs_debug_live_allocations() == start


def test_refiner_regrow_releases_what_it_replaces(lib):
    start = lib.hs_debug_live_allocations()
    fresh = _refiner(lib, n=40)
    n_fresh = lib.hs_debug_live_allocations() - start
    lib.hs_refiner_destroy(fresh)
    assert lib.hs_debug_live_allocations() == start
    grown = _refiner(lib, n=5)
    _refiner_points(lib, grown, 40)
    assert lib.hs_debug_live_allocations() - start == n_fresh
    lib.hs_refiner_destroy(grown)
    assert lib.hs_debug_live_allocations() == start


def test_one_shot_calls_leave_nothing(lib):
    from hslam_amd.pyr import dir_pyramid
    start = lib.hs_debug_live_allocations()
    img = np.random.default_rng(9).random((H, W), dtype=np.float32) * 255
    dir_pyramid(img, 2)
    assert lib.hs_debug_live_allocations() == start
    fn = lib.hs_debug_fastmath
    fn.argtypes, fn.restype = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int
    a, b, out = np.array([1, 2, 3], np.float32), np.array([4, 5, 6], np.float32), np.zeros((3, 4), np.float32)
    _ok(lib, fn(3, _p(a), _p(b), _p(out)))
    assert np.allclose(out[:, 1], a / b, rtol=1e-6, atol=0)
    assert lib.hs_debug_live_allocations() == start
