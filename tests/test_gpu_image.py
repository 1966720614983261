"""include/hs_image.h on the device: one camera frame built once (hs_k_img_levels, hs_k_img_grads) and handed to every
consumer device to device.  Bar: bit-identity with the existing chain (hs_undistorter_apply, then the pyramid of
hs_dir_pyramid / the oracle) and with each consumer's existing entry; expected values never come from hs_image."""
import ctypes as C
import gc

import numpy as np
import pytest

from undist_cases import CASES, gamma_G, lib_calib, random_vignette

pytestmark = pytest.mark.gpu

W, H, LEVELS = 320, 240, 4          # the consumers' size: undist_cases' "chain" calibration
K = np.array([[128.0, 0, 159.5], [0, 127.2, 119.5], [0, 0, 1.0]])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def frame_u8(name, seed=11):
    c = CASES[name]
    return np.random.default_rng(seed).integers(0, 256, size=(c["h_in"], c["w_in"]), dtype=np.uint8)


def passthrough(w, h):
    from hslam_amd.undistort import Undistorter, make_calib
    return Undistorter(make_calib("Pinhole", w, h, w, h, (0.6 * w, 0.6 * w, 0.5 * w - 0.5, 0.5 * h - 0.5), (0.0,), "none"))


def expected_levels(fimg, n_levels):
    """The existing chain's pyramid of fImgL: the oracle and the device entry, which must agree."""
    from hslam_amd.pyr import dir_pyramid as dev
    from oracle_ffi import dir_pyramid as oracle
    pd, gd = dev(fimg, n_levels)
    po, go = oracle(fimg, n_levels)
    for l in range(n_levels):
        assert same(pd[l], po[l]) and same(gd[l], go[l]), l
    return pd, gd


def check_levels(im, fimg, img8):
    pyr, grads = expected_levels(fimg, im.n_levels)
    for l in range(im.n_levels):
        if l == 0 and img8 is not None:
            d, g, c = im.get(0, img8=True)
            assert same(c, img8)
        else:
            d, g = im.get(l)
        assert d.shape == (im.H >> l, im.W >> l, 3)
        for lane in range(3):
            assert same(d[..., lane], pyr[l][..., lane]), (l, lane)
        assert same(g, grads[l]), l


# ---- 1. pyramid and cvImgL

@pytest.mark.parametrize("mode", ["none", "gamma", "vignette", "both"])
def test_small_usek_modes(mode):
    from hslam_amd.image import DeviceImage
    from hslam_amd.undistort import Undistorter
    c = CASES["small_usek"]
    u = Undistorter(lib_calib("small_usek"))
    u.set_photometric(gamma_G() if mode in ("gamma", "both") else None,
                      random_vignette((c["h_in"], c["w_in"])) if mode in ("vignette", "both") else None)
    raw = frame_u8("small_usek")
    fimg, img8 = u.undistort(raw)
    im = DeviceImage(c["w_out"], c["h_out"], 4)
    im.set_u8(u, raw)
    check_levels(im, fimg, img8)
    assert im.last_stats() > 0
    im.close()
    u.close()


def test_odd_size_crop():
    from hslam_amd.image import DeviceImage
    from hslam_amd.undistort import Undistorter
    c = CASES["odd_crop"]
    u = Undistorter(lib_calib("odd_crop"))
    u.set_photometric(gamma_G(), None)
    raw = frame_u8("odd_crop")
    fimg, img8 = u.undistort(raw)
    im = DeviceImage(c["w_out"], c["h_out"], 3)
    im.set_u8(u, raw)
    check_levels(im, fimg, img8)
    # a second frame into the same levels
    raw2 = np.ascontiguousarray(raw[::-1])
    fimg2, img82 = u.undistort(raw2)
    im.set_u8(u, raw2)
    check_levels(im, fimg2, img82)
    im.close()
    u.close()


@pytest.mark.parametrize("w, h, levels", [(104, 72, 4),     # 13 x 9 at the top: no multiple of any tile
                                          (101, 75, 3),     # odd at levels 0 and 2: the unused last column and row
                                          (1232, 368, 5)])  # one full size
def test_passthrough_sizes(w, h, levels):
    from hslam_amd.image import DeviceImage
    u = passthrough(w, h)
    raw = np.random.default_rng(w).integers(0, 256, size=(h, w), dtype=np.uint8)
    fimg, img8 = u.undistort(raw)
    assert same(fimg, raw.astype(np.float32))
    im = DeviceImage(w, h, levels)
    im.set_u8(u, raw)
    check_levels(im, fimg, img8)
    # the same image object, a second frame: nothing of the first is left
    raw2 = np.ascontiguousarray(raw[::-1, ::-1])
    fimg2, img82 = u.undistort(raw2)
    im.set_u8(u, raw2)
    check_levels(im, fimg2, img82)
    im.close()
    u.close()


@pytest.fixture(scope="module")
def track_scene():
    from hslam_amd.scene import make_track_scene
    return make_track_scene(n_points=400, width=W, height=H, n_levels=LEVELS, K=K)


def test_set_raw_levels_and_no_cvimg(track_scene):
    from hslam_amd._lib import HsError
    from hslam_amd.extract import FeatureExtractor
    from hslam_amd.flow import KeypointFlow
    from hslam_amd.image import DeviceImage
    from hslam_amd.select import PixelSelector
    import extract_cases as xc
    fimg = np.ascontiguousarray(track_scene.new_pyr[0][..., 0])
    im = DeviceImage(W, H, LEVELS)
    im.set_raw(fimg)
    check_levels(im, fimg, None)
    with pytest.raises(HsError, match=r"\(-5\).*cvImgL"):
        im.get(0, img8=True)
    sel = PixelSelector(W, H)
    sel.makeMapsRaw(fimg, 0, 600)
    ex = FeatureExtractor(W, H, 4000, xc.random_pattern())
    with pytest.raises(HsError, match=r"\(-5\).*cvImgL"):
        ex.extract_image(sel, im)
    fl = KeypointFlow(W, H, 10)
    fl.set_first(np.zeros((H, W), np.uint8), np.array([[50.0, 50.0]], np.float32))
    with pytest.raises(HsError, match=r"\(-5\).*cvImgL"):
        fl.track_image(im, 7)
    # a u8 frame after it brings cvImgL back
    u = passthrough(W, H)
    raw = np.clip(np.rint(fimg), 0, 255).astype(np.uint8)
    im.set_u8(u, raw)
    f2, i2 = u.undistort(raw)
    check_levels(im, f2, i2)
    for o in (ex, fl, im, u):
        o.close()


# ---- 2. each consumer against the entry it replaces

@pytest.fixture(scope="module")
def chain():
    """The 352 x 264 -> 320 x 240 calibration with a gamma table, two textured raw frames (the second the first
    moved by (1.5, 0.5) px) and what the existing chain makes of them."""
    import flow_cases as fc
    from hslam_amd.undistort import Undistorter
    c = CASES["chain"]
    u = Undistorter(lib_calib("chain"))
    u.set_photometric(gamma_G(), None)
    f0 = fc.field(c["w_in"], c["h_in"], seed=61)
    raws = [fc.crop8(f0), fc.crop8(np.clip(fc.ndimage.shift(f0, (0.5, 1.5), order=3, mode="nearest"), 0, 255))]
    outs = [u.undistort(r) for r in raws]
    yield u, raws, [o[0] for o in outs], [o[1] for o in outs]
    u.close()


@pytest.fixture()
def image(chain):
    from hslam_amd.image import DeviceImage
    im = DeviceImage(W, H, LEVELS)
    yield im
    im.close()


def hip():
    """The HIP runtime the product library has already loaded into this process."""
    with open("/proc/self/maps") as maps:
        path = next(line.split()[-1] for line in maps if "libamdhip64" in line)
    lib = C.CDLL(path)
    lib.hipMemcpy.argtypes, lib.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    lib.hipDeviceSynchronize.argtypes, lib.hipDeviceSynchronize.restype = [], C.c_int
    return lib


def tracker_texels(t, n_levels):
    """The tracker's frame, every level as (h, w, 4) float32, read where hs_tracker_frame_texels says it lies."""
    lib = hip()
    assert lib.hipDeviceSynchronize() == 0
    out = []
    for l in range(n_levels):
        a = np.empty((t.hl[l], t.wl[l], 4), np.float32)
        assert lib.hipMemcpy(a.ctypes.data, t.frame_texels(l), a.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        out.append(a)
    return out


def test_tracker(chain, image, track_scene):
    from hslam_amd.track import CoarseTracker
    u, raws, fimgs, _ = chain
    s = track_scene
    a = CoarseTracker(W, H, s.K4, LEVELS)
    b = CoarseTracker(W, H, s.K4, LEVELS)
    for t in (a, b):
        t.setCoarseTrackingRef(s.ref_pyr, s.ref_exposure, s.ref_aff, s.pt_u, s.pt_v, s.pt_idepth, s.pt_hdi)
    a.setNewFrameU8(u, raws[0], s.new_exposure)
    image.set_u8(u, raws[0])
    b.setNewFrameImage(image, s.new_exposure)
    for lvl in range(LEVELS):
        ra, Ha, ba_, na = a.calcRes(lvl, s.T_true, s.aff_true, 20.0)
        rb, Hb, bb_, nb = b.calcRes(lvl, s.T_true, s.aff_true, 20.0)
        assert na == nb and same(ra, rb) and same(Ha, Hb) and same(ba_, bb_), lvl
    ta, tb = tracker_texels(a, LEVELS), tracker_texels(b, LEVELS)
    pyr, _ = expected_levels(fimgs[0], LEVELS)
    for lvl in range(LEVELS):
        assert same(ta[lvl], tb[lvl]), lvl
        assert same(tb[lvl][..., :3], pyr[lvl]) and not tb[lvl][..., 3].any(), lvl
    a.close()
    b.close()


@pytest.fixture(scope="module")
def trace_scene():
    from hslam_amd.scene import make_trace_scene
    return make_trace_scene(n_points=500, n_hosts=4, width=W, height=H, seed=9)


def test_tracer_frame(chain, image, trace_scene):
    from hslam_amd.trace import ImmatureTracer
    u, raws, _, _ = chain
    s = trace_scene
    a = ImmatureTracer(W, H, s.n_points)
    b = ImmatureTracer(W, H, s.n_points)
    for t in (a, b):
        for i, img in enumerate(s.host_imgs):
            t.set_host_image(i, img)
        t.add_points(s.pt_host, s.pt_u, s.pt_v)
    a.set_frame_u8(u, raws[0])
    image.set_u8(u, raws[0])
    b.set_frame_image(image)
    assert same(a.traceNewCoarse(s.KRKi, s.Kt, s.aff), b.traceNewCoarse(s.KRKi, s.Kt, s.aff))
    pa, pb = a.points(), b.points()
    for k in pa:
        assert np.array_equal(pa[k], pb[k], equal_nan=True), k
    a.close()
    b.close()


def test_tracer_host_slot(chain, image):
    import flow_cases as fc
    from hslam_amd.pyr import dir_pyramid
    from hslam_amd.trace import ImmatureTracer
    u, raws, fimgs, _ = chain
    dirpyr0 = dir_pyramid(fimgs[1], 1)[0][0]           # the host DirPyr[0] an integrator would have built
    pts = fc.interior_points(W, H, 300, seed=5)
    a = ImmatureTracer(W, H, 300)
    b = ImmatureTracer(W, H, 300)
    a.set_host_image(3, dirpyr0)
    image.set_u8(u, raws[1])
    b.set_host_image_from(3, image)
    for t in (a, b):
        t.add_points(np.full(300, 3, np.int32), pts[:, 0], pts[:, 1])
    pa, pb = a.points(), b.points()
    for k in ("color", "weights", "gradH", "energyTH"):
        assert same(pa[k], pb[k]), k
    assert np.any(pa["gradH"] != 0)
    a.close()
    b.close()


def test_selector_two_frames(chain, image):
    from hslam_amd.select import PixelSelector
    u, raws, fimgs, _ = chain
    a, b = PixelSelector(W, H), PixelSelector(W, H)
    for k in range(2):                                  # the potential of frame 0 carries into frame 1
        ma, na = a.makeMapsRaw(fimgs[k], k, 600)
        image.set_u8(u, raws[k])
        mb, nb = b.makeMapsImage(image, k, 600)
        assert na == nb > 100 and same(ma, mb), k
        assert a.currentPotential == b.currentPotential
        assert a.last_stats()[1] == b.last_stats()[1]


def test_extractor(chain, image):
    import extract_cases as xc
    from hslam_amd.extract import FeatureExtractor
    from hslam_amd.select import PixelSelector
    u, raws, fimgs, _ = chain
    sel = PixelSelector(W, H)
    sel.makeMapsRaw(fimgs[0], 0, 600)
    pat = xc.random_pattern()
    a, b = FeatureExtractor(W, H, 4000, pat), FeatureExtractor(W, H, 4000, pat)
    na = a.extract_u8(sel, u, raws[0])
    image.set_u8(u, raws[0])
    nb = b.extract_image(sel, image)
    assert na == nb > 50
    ga, gb = a.get(blurred=True), b.get(blurred=True)
    for k in ga:
        assert same(ga[k], gb[k]), k
    a.close()
    b.close()


def test_flow(chain, image):
    import flow_cases as fc
    from hslam_amd.flow import KeypointFlow
    u, raws, _, img8s = chain
    pts = fc.interior_points(W, H, 150, seed=62)
    a, b = KeypointFlow(W, H, 150), KeypointFlow(W, H, 150)
    for f in (a, b):
        f.set_first(img8s[0], pts)
    na = a.track_u8(u, raws[1], 7)
    image.set_u8(u, raws[1])
    nb = b.track_image(image, 7)
    ga, gb = a.get(), b.get()
    for k in ga:
        assert same(ga[k], gb[k]), k
    assert na == nb > 75
    a.close()
    b.close()


@pytest.fixture(scope="module")
def ba_scene():
    from hslam_amd.scene import make_ba_scene
    return make_ba_scene(n_points=60, n_frames=3, width=W, height=H, K=K, seed=5)


def ba_outputs(win):
    e = win.linearizeAll(reset=True)
    return e, win.residuals()


def committed_window(scene):
    from hslam_amd.ba import BAWindow
    win = BAWindow(scene)
    win.linearizeAll(reset=True)          # the window's own images are on the device before one of them changes
    return win


def test_ba_window_image(ba_scene):
    from hslam_amd.ba import BAWindow
    from hslam_amd.image import DeviceImage
    s = ba_scene
    u = passthrough(W, H)
    raw = np.clip(np.rint(s.pyramids[2][0][..., 0]), 0, 255).astype(np.uint8)   # the newest frame as a camera saw it
    fimg, _ = u.undistort(raw)
    a, b = BAWindow(s), BAWindow(s)
    e0, _ = ba_outputs(a)                 # both windows are committed before their images change
    assert ba_outputs(b)[0] == e0
    a.set_frame_image_raw(2, fimg)
    im = DeviceImage(W, H, 1)
    im.set_u8(u, raw)
    b.set_frame_image_from(2, im)
    (ea, ra), (eb, rb) = ba_outputs(a), ba_outputs(b)
    assert ea == eb and ea != e0          # the quantised image changed the energy, the same way in both
    for k in ra:
        assert same(ra[k], rb[k]), k
    assert ra["state"].size > 60 and np.any(ra["energy"] != 0)
    for o in (a, b, im, u):
        o.close()


# ---- 3. ordering on the device, no host wait between a hand-off and the next set

def test_back_to_back_frames_reach_their_consumers():
    from hslam_amd.ba import BAWindow
    from hslam_amd.image import DeviceImage
    from hslam_amd.pyr import dir_pyramid
    from hslam_amd.scene import make_ba_scene
    from hslam_amd.trace import ImmatureTracer
    from hslam_amd.track import CoarseTracker
    import flow_cases as fc
    w, h, levels = 640, 480, 4
    s = make_ba_scene(n_points=60, n_frames=3, seed=5)
    u = passthrough(w, h)
    raws = [np.clip(np.rint(s.pyramids[k][0][..., 0]), 0, 255).astype(np.uint8) for k in (2, 1)]   # A, B
    fimgs = [r.astype(np.float32) for r in raws]
    k4 = (256.0, 254.4, 319.5, 239.5)
    pts = fc.interior_points(w, h, 200, seed=8)
    eye = np.eye(3, dtype=np.float32).reshape(1, 9)
    Kt, aff = np.array([[0.8, 0.1, 0.0]], np.float32), np.array([[1.0, 0.0]], np.float32)

    def new_tracer():
        t = ImmatureTracer(w, h, 200)
        t.set_host_image(0, s.pyramids[0][0])
        t.add_points(np.zeros(200, np.int32), pts[:, 0], pts[:, 1])
        return t

    # what each frame leaves in a consumer, by the existing entries
    want = []
    for f in fimgs:
        pyr, _ = dir_pyramid(f, levels)
        trc = new_tracer()
        trc.set_frame_raw(f)
        counts = trc.traceNewCoarse(eye, Kt, aff)
        win = committed_window(s)
        win.set_frame_image_raw(2, f)
        want.append(dict(pyr=pyr, counts=counts, points=trc.points(), ba=ba_outputs(win)))
        trc.close()
        win.close()
    assert any(not same(want[0]["points"][key], want[1]["points"][key]) for key in want[0]["points"])
    assert want[0]["ba"][0] != want[1]["ba"][0]

    im = DeviceImage(w, h, levels)
    sets = [dict(trk=CoarseTracker(w, h, k4, levels), trc=new_tracer(), ba=committed_window(s)) for _ in range(2)]
    for rnd in range(3):
        order = (0, 1) if rnd % 2 == 0 else (1, 0)
        for cs, k in zip(sets, order):         # set, three hand-offs, and at once the next set
            im.set_u8(u, raws[k])
            cs["trk"].setNewFrameImage(im, 1.0)
            cs["trc"].set_frame_image(im)
            cs["ba"].set_frame_image_from(2, im)
            cs["frame"] = k
    for cs in sets:
        w_ = want[cs["frame"]]
        tex = tracker_texels(cs["trk"], levels)
        for l in range(levels):
            assert same(tex[l][..., :3], w_["pyr"][l]) and not tex[l][..., 3].any(), (cs["frame"], l)
        assert same(cs["trc"].traceNewCoarse(eye, Kt, aff), w_["counts"])
        got = cs["trc"].points()
        for key in got:
            assert np.array_equal(got[key], w_["points"][key], equal_nan=True), key
        e, r = ba_outputs(cs["ba"])
        assert e == w_["ba"][0]
        for key in r:
            assert same(r[key], w_["ba"][1][key]), key
    assert sets[0]["frame"] == 0 and sets[1]["frame"] == 1      # round 3 ran in the first order
    for cs in sets:
        for key in ("trk", "trc", "ba"):
            cs[key].close()
    im.close()
    u.close()


# ---- 4. errors

def test_errors_leave_the_consumer_alone(chain, track_scene):
    import extract_cases as xc
    from hslam_amd._lib import HsError, check, ptr
    from hslam_amd.ba import BAWindow
    from hslam_amd.extract import FeatureExtractor
    from hslam_amd.image import DeviceImage
    from hslam_amd.select import PixelSelector
    from hslam_amd.trace import ImmatureTracer
    from hslam_amd.track import CoarseTracker
    u, raws, fimgs, _ = chain
    s = track_scene
    t = CoarseTracker(W, H, s.K4, LEVELS)
    t.set_scene(s)
    before = t.calcRes(0, s.T_true, s.aff_true, 20.0)
    empty = DeviceImage(W, H, LEVELS)
    trc = ImmatureTracer(W, H, 8)
    sel = PixelSelector(W, H)
    with pytest.raises(HsError, match=r"\(-5\).*no frame"):      # before any set
        t.setNewFrameImage(empty, 1.0)
    with pytest.raises(HsError, match=r"\(-5\).*no frame"):
        trc.set_frame_image(empty)
    with pytest.raises(HsError, match=r"\(-5\).*no frame"):
        trc.set_host_image_from(0, empty)
    with pytest.raises(HsError, match=r"\(-5\).*no frame"):
        sel.makeMapsImage(empty, 0, 600)
    with pytest.raises(HsError, match=r"\(-5\).*no frame"):
        empty.get(0)
    with pytest.raises(HsError, match=r"\(-1\).*slot"):
        trc.set_host_image_from(99, empty)
    with pytest.raises(HsError, match=r"\(-1\).*point on a host slot"):    # the failed entry made no slot
        trc.add_points([0], [20.0], [20.0])
    # another size
    pu = passthrough(W + 32, H)
    wide = DeviceImage(W + 32, H, LEVELS)
    wide.set_u8(pu, np.zeros((H, W + 32), np.uint8))
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        t.setNewFrameImage(wide, 1.0)
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        trc.set_frame_image(wide)
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        sel.makeMapsImage(wide, 0, 600)
    win = BAWindow(camera=(W, H, LEVELS, K), capacity=16)
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        win.set_frame_image_from(0, wide)
    # too few levels
    two = DeviceImage(W, H, 2)
    two.set_u8(u, raws[0])
    with pytest.raises(HsError, match=r"\(-1\).*levels"):
        sel.makeMapsImage(two, 0, 600)
    with pytest.raises(HsError, match=r"\(-1\).*levels"):
        t.setNewFrameImage(two, 1.0)
    ex = FeatureExtractor(W, H, 100, xc.random_pattern())
    with pytest.raises(HsError, match=r"\(-5\).*no map"):        # none of the failed calls left a map in the selector
        ex.extract_image(sel, two)
    ex.close()
    with pytest.raises(HsError, match=r"\(-1\).*bad level"):
        two.get(2)
    with pytest.raises(HsError, match=r"\(-1\).*level 0"):
        check(two.lib.hs_image_get(two.h, 1, None, None, ptr(np.empty((H, W), np.uint8))))
    # an undistorter of another output size
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        wide.set_u8(u, raws[0])
    # the tracker still holds the scene's frame
    after = t.calcRes(0, s.T_true, s.aff_true, 20.0)
    assert before[3] == after[3] and all(same(x, y) for x, y in zip(before[:3], after[:3]))
    for o in (t, trc, empty, wide, two, win, pu):
        o.close()


# ---- 5. lifetime

def test_destroy_returns_every_allocation(chain):
    from hslam_amd._lib import load
    from hslam_amd.image import DeviceImage
    from hslam_amd.trace import ImmatureTracer
    u, raws, fimgs, _ = chain
    lib = load()
    lib.hs_debug_live_allocations.argtypes, lib.hs_debug_live_allocations.restype = [], C.c_longlong
    gc.collect()
    trc = ImmatureTracer(W, H, 8)
    start = lib.hs_debug_live_allocations()
    im = DeviceImage(W, H, LEVELS)
    assert lib.hs_debug_live_allocations() > start
    im.set_u8(u, raws[0])                 # the raw staging, pinned and device
    im.set_raw(fimgs[0])                  # the float staging
    trc.set_frame_image(im)               # a consumer's event outstanding at destroy
    im.close()
    assert lib.hs_debug_live_allocations() == start
    h = C.c_void_p(1)
    assert lib.hs_image_create(C.byref(h), 4096, W, H, LEVELS) == -1      # no such device
    assert not h.value and lib.hs_debug_live_allocations() == start
    trc.close()
