"""The initializer closed on the device: the draw of mvSets (hs_twoview_draw, hs_twoview_fit_flow_drawn) against the
model of include/hs_twoview.h's generator and draw (tests/initializer_ref.py), hs_flow_mean_flow_device against
hs_flow_mean_flow, and the hslam_amd.initializer.Initializer driver against a hand-written twin that makes the same brick
calls with the sets drawn by the model and uploaded.  Every comparison is bit for bit; expected sets and states never
come from the device.

The driver's four frames (first, first again, the 0.15 m baseline, the 0.25 m baseline of one world) were run through
the numpy models (tests/flow_ref.py Matcher, tests/twoview_ref.py fit, initializer_ref) on the CPU first: with seed 0
they take the exits first / stationary (mean flow 0.0) / fit_failed (259 matches, mean flow 8.51, why 3) / success (230
matches after the untriangulated keys left, 265 triangulated, mean flow 3.57)."""
import ctypes as C
import functools
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from initializer_ref import CvRng, draw_sets_cv  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
K4_320 = np.array([128.0, 127.2, 159.5, 119.5])
HIGH_SEED = 0x1234567800000005                                       # a non-zero high word


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def state_words(state):
    return [state & 0xFFFFFFFF, state >> 32]


def masked(res):
    """The 128-byte record without the two words that carry the generator's state (reserved[0], reserved[1])."""
    b = bytearray(bytes(res))
    b[104:112] = bytes(8)
    return bytes(b)


# ---- 1. the draw

@functools.lru_cache(maxsize=None)
def draw_status(n):
    st = np.ones(n, np.uint8)
    if n == 9:
        st[4] = 0
    elif n == 67:
        st[[0, 13, 63, 64, 66]] = 0
    elif n == 300:
        st[60:68] = 0                                                # runs of bad keys across the wave boundary 63 / 64
        st[250:261] = 0                                              # and across 255 / 256
        st[299] = 0
    elif n == 2049:                                                  # more than one chunk of the list's block
        st[np.random.default_rng(3).choice(n, 205, replace=False)] = 0
    st.setflags(write=False)
    return st


@pytest.fixture(scope="module")
def tv():
    from hslam_amd.twoview import TwoViewFit
    t = TwoViewFit(2049, K4_320)
    yield t
    t.close()


@pytest.mark.parametrize("seed", [0, HIGH_SEED])
@pytest.mark.parametrize("n, n_sets", [(8, 1), (8, 3), (9, 5), (67, 200), (300, 200), (2049, 256)])
def test_draw_matches_the_model(tv, n, n_sets, seed):
    st = draw_status(n)
    model = CvRng(seed)
    want = draw_sets_cv(st, n_sets, model)
    tv.rng_seed(seed)
    assert tv.rng_state() == (seed or 0xFFFFFFFF)
    sets, m = tv.draw(st, n_sets)
    assert m == int(st.sum())
    assert same(sets, want), np.flatnonzero((sets != want).any(axis=1))[:8]
    assert tv.rng_state() == model.state
    if m == 8:                                                       # the draw that is not taken
        c = CvRng(seed)
        c.skip(7 * n_sets)
        assert tv.rng_state() == c.state


def test_two_draws_continue_one_sequence_and_skip_is_next(tv):
    st = draw_status(300)
    model = CvRng(0)
    want = draw_sets_cv(st, 50, model)
    tv.rng_seed(0)
    a, _ = tv.draw(st, 20)
    b, _ = tv.draw(draw_status(300), 30)
    assert same(np.concatenate([a, b]), want) and tv.rng_state() == model.state
    for k in (0, 1, 6000):
        tv.rng_skip(k)
        model.skip(k)
        assert tv.rng_state() == model.state
    c, _ = tv.draw(draw_status(67), 7)
    assert same(c, draw_sets_cv(draw_status(67), 7, model)) and tv.rng_state() == model.state


# ---- 2. refusals

def seven_good_flow():
    """12 keys of which exactly 7 track (the model: tests/flow_ref.py Matcher gives n_good 7): the other five lie far
    outside the image."""
    import flow_cases as fc
    from hslam_amd.flow import KeypointFlow
    a, b, pts, _, _ = fc.shift_case(0)
    keys = np.concatenate([pts[:7], np.full((5, 2), -100.0, f32)]).astype(f32)
    fl = KeypointFlow(96, 80, 12)
    fl.set_first(a, keys)
    assert fl.track(b, 7) == 7
    return fl


def test_refusals_change_nothing():
    from hslam_amd._lib import HsError
    from hslam_amd.twoview import TwoViewFit
    from test_gpu_twoview import tracked_flow
    s, fl = tracked_flow()
    t = TwoViewFit(300, s.K4)
    assert t.fit_flow_drawn(fl, 200).ok == 1                        # seed 0, as create leaves it
    want, want_g, want_rt, want_sets, state = bytes(t.last_result()), t.get(), t.get_rt(), t.sets(), t.rng_state()

    def unchanged(record=True):
        assert t.rng_state() == state
        assert not record or bytes(t.last_result()) == want
        g, rt = t.get(), t.get_rt()
        assert all(same(g[k], want_g[k]) for k in g) and all(same(rt[k], want_rt[k]) for k in rt)
        assert same(t.sets(), want_sets)

    seven = np.zeros(20, np.uint8)
    seven[[0, 3, 4, 9, 12, 18, 19]] = 1
    for st, n_sets, pat in ((seven, 5, r"\(-1\).*status"), (np.ones(50, np.uint8), 0, r"\(-1\).*n_sets"),
                            (np.ones(50, np.uint8), 257, r"\(-1\).*n_sets"), (np.ones(301, np.uint8), 5, r"\(-1\).*capacity"),
                            (np.ones(7, np.uint8), 5, r"\(-1\).*capacity")):
        with pytest.raises(HsError, match=pat):
            t.draw(st, n_sets)
        unchanged()
    for n_sets in (0, 257):
        with pytest.raises(HsError, match=r"\(-1\).*n_sets"):
            t.fit_flow_drawn(fl, n_sets)
        unchanged()
    sets, m = t.draw(np.ones(50, np.uint8), 3)                       # a draw that works moves the state, not the fit
    state = t.rng_state()
    unchanged()
    # fewer than 8 matched keys: not an error, a refused fit; the generator does not move
    fl7 = seven_good_flow()
    res = t.fit_flow_drawn(fl7, 50)
    assert (res.ok, res.why, res.model, res.best_h, res.best_f, res.best_rt, res.n_rt) == (0, 5, -1, -1, -1, -1, 0)
    assert [w & 0xFFFFFFFF for w in list(res.reserved)[:2]] == state_words(state) and not any(list(res.reserved)[2:])
    assert bytes(t.last_result()) == bytes(res)
    unchanged(record=False)
    from hslam_amd.refine import DirectRefinement
    r = DirectRefinement.bare(s.width, s.height, s.K4)
    with pytest.raises(HsError, match=r"\(-5\)"):                    # the last fit did not succeed
        r.set_points_twoview(fl, t)
    for o in (r, t, fl, fl7):
        o.close()


# ---- 3. the fit with drawn sets is the fit with the same sets uploaded

@pytest.mark.parametrize("seed", [0, HIGH_SEED])
def test_drawn_fit_is_the_uploaded_fit(seed):
    from hslam_amd.refine import DirectRefinement
    from hslam_amd.twoview import TwoViewFit
    from test_gpu_init import assert_same
    from test_gpu_twoview import tracked_flow
    s, fl = tracked_flow()
    good = fl.get()["good"]
    model = CvRng(seed)
    want_sets = draw_sets_cv(good, 200, model)
    a, b = TwoViewFit(300, s.K4), TwoViewFit(512, s.K4)
    a.rng_seed(seed)
    ra = a.fit_flow_drawn(fl, 200)
    assert same(a.sets(), want_sets)
    assert a.rng_state() == model.state
    assert [w & 0xFFFFFFFF for w in list(ra.reserved)[:2]] == state_words(model.state) and not any(list(ra.reserved)[2:])
    rb = b.fit_flow(fl, want_sets)
    assert same(b.sets(), want_sets) and not any(rb.reserved) and b.rng_state() == 0xFFFFFFFF
    assert ra.ok == 1 and masked(ra) == masked(rb) == bytes(rb)
    assert_same(a.get(), b.get())
    assert_same(a.get_rt(), b.get_rt())
    p, q = DirectRefinement.bare(s.width, s.height, s.K4), DirectRefinement.bare(s.width, s.height, s.K4)
    for r_ in (p, q):
        r_.set_frames(s.img1, s.img2, s.expo1, s.expo2)
    p.set_points_twoview(fl, a)
    q.set_points_twoview(fl, b)
    assert_same(p.points(), q.points())
    assert same(p.videpth(), q.videpth()) and (p.videpth() > 0).sum() == ra.n_triangulated
    for o in (p, q, a, b, fl):
        o.close()


# ---- 4. the mean flow

def both_means(fl):
    a, b = fl.mean_flow_device(), fl.mean_flow()
    print(f"mean flow: device {a!r} host {b!r}")
    return f32(a), f32(b)


@pytest.mark.parametrize("n", [7, 33, 300])
def test_mean_flow_device_is_mean_flow(n):
    from hslam_amd._lib import HsError
    from hslam_amd.flow import KeypointFlow
    from test_gpu_init import fimgs, img8_of, scene
    s = scene(n)
    f1, f2 = fimgs(s)
    fl = KeypointFlow(s.width, s.height, n)
    fl.set_first(img8_of(f1), np.stack([s.u, s.v], 1).astype(f32))
    with pytest.raises(HsError, match=r"\(-5\).*track"):             # before a track
        fl.mean_flow_device()
    n_good = fl.track(img8_of(f2), 7)
    a, b = both_means(fl)
    if n_good:
        assert a.tobytes() == b.tobytes() and np.isfinite(b) and b >= 0
    else:
        assert np.isnan(a) and np.isnan(b)
    fl.close()


def test_mean_flow_device_over_more_than_one_chunk():
    """2049 random keys on tests/test_gpu_flow.py's field, some of them lost, over two tracks of about 2.6 px: the
    truncating sum differs from the float sum here.  The model's value (tests/flow_ref.py) is the third witness."""
    import flow_cases as fc
    import flow_ref as ref
    from hslam_amd.flow import KeypointFlow
    frames = fc.chain_frames()
    pts = fc.coverage_points(96, 80, seed=7, n=2042)
    assert len(pts) == 2049
    fl = KeypointFlow(96, 80, 2049)
    fl.set_first(frames[0], pts)
    for img in frames[1:]:
        n_good = fl.track(img, 7)
        assert 1024 < n_good < 2049
        a, b = both_means(fl)
        g = fl.get()
        assert a.tobytes() == b.tobytes() == f32(ref.mean_flow(g["prev_xy"], g["xy"], g["good"])).tobytes()
        d = (g["prev_xy"] - g["xy"])[g["good"] != 0].astype(np.float64)
        assert abs(float(np.hypot(d[:, 0], d[:, 1]).mean()) - float(b)) > 0.1       # the truncation shows
    # every key lost: NaN from both
    fl.set_first(frames[0], np.full((9, 2), -100.0, f32))
    assert fl.track(frames[1], 7) == 0
    a, b = both_means(fl)
    assert np.isnan(a) and np.isnan(b)
    fl.close()


# ---- 5. the driver against its twin

@functools.lru_cache(maxsize=None)
def sequence():
    """(frames, keys, scene): the first frame, the first frame again, the second view at the 0.15 m and at the 0.25 m
    baseline.  make_refine_scene draws the world, the first view and the keys before it uses `trans`, so both scenes
    share them (asserted)."""
    from test_gpu_init import fimgs, img8_of
    from test_gpu_twoview import pair_scene
    s15, s25 = pair_scene(0.15), pair_scene(0.25)
    a, b, c = img8_of(fimgs(s15)[0]), img8_of(fimgs(s15)[1]), img8_of(fimgs(s25)[1])
    assert same(a, img8_of(fimgs(s25)[0])) and same(s15.u, s25.u) and same(s15.v, s25.v)
    keys = np.stack([s15.u, s15.v], 1).astype(f32)
    return (a, a, b, c), keys, s15


def identity_undistorter(s):
    """The raw frame is the undistorted frame: every remap tap at an integer source pixel."""
    from hslam_amd.undistort import Undistorter, make_calib
    u = Undistorter(make_calib("Pinhole", s.width, s.height, s.width, s.height, s.K4, (0.0,), "none"))
    yy, xx = np.mgrid[0:s.height, 0:s.width]
    u.set_remap(xx.astype(f32), yy.astype(f32))
    return u


def window_of(s):
    from hslam_amd.ba import BAWindow
    return BAWindow(camera=(s.width, s.height, 1, s.K), capacity=400)


def run_driver(seed):
    from hslam_amd.initializer import Initializer
    from test_gpu_init import window_readbacks
    frames, keys, s = sequence()
    u = identity_undistorter(s)
    ini = Initializer(s.width, s.height, s.K4, 300)
    ini.reset_rng(seed)
    returned = [ini.Initialize(img, u, 1.0, keys=keys) for img in frames]
    ba = window_of(s)
    why, hd, pose = ini.init_window(ba)
    ba.makeIDX()
    o = dict(returned=returned, history=ini.history, record=bytes(ini.result), pose=ini.pose, vid=ini.videpth(),
             good=ini.good, why=why, n_seeded=np.array([len(hd)]), img8=ini.first_image.get(0, img8=True)[2],
             fails=ini.NumFails)
    o.update(window_readbacks(ba))
    for x in (ba, ini, u):
        x.close()
    return o


def run_twin(seed):
    """Initialize and InitFromInitializer written out over the bricks, with the host's part of the parent's path: the
    status read back, the sets drawn by the model and uploaded, the mean flow on the host."""
    from hslam_amd.ba import make_frame
    from hslam_amd.flow import KeypointFlow
    from hslam_amd.image import DeviceImage
    from hslam_amd.refine import DirectRefinement
    from hslam_amd.scene import se3_data
    from hslam_amd.twoview import TwoViewFit
    from test_gpu_init import IDENTITY, window_readbacks
    frames, keys, s = sequence()
    u = identity_undistorter(s)
    first_im, im = DeviceImage(s.width, s.height, 4), DeviceImage(s.width, s.height, 4)
    fl, tv, r = KeypointFlow(s.width, s.height, 300), TwoViewFit(300, s.K4), DirectRefinement.bare(s.width, s.height, s.K4)
    rng = CvRng(seed)
    n = len(keys)
    has_first, fails, actions, states, returned = False, 0, [], [], []
    res = pose = good = None

    def one(img):
        nonlocal has_first, fails, first_im, im, res, pose, good
        im.set_u8(u, img)
        if fails > 40:
            has_first, fails = False, 0
        if not has_first:
            if n > 100:
                fl.set_first_image(im, keys)
                r.set_first_image(im, 1.0)
                first_im, im = im, first_im
                rng.skip(3 * n)                                      # ColorVec
                has_first = True
                return "first"
            return "no_frame"
        if not n > 100:
            has_first = False
            return "reset_features"
        nmatches = fl.track_image(im, 7)
        if f32(nmatches) < f32(0.2) * f32(n):
            has_first = False
            return "reset_matches"
        if fl.mean_flow() < f32(2.0):
            return "stationary"
        sets = draw_sets_cv(fl.get()["good"], 200, rng)
        res = tv.fit_flow(fl, sets)
        if not res.ok:
            fails += 1
            return "fit_failed"
        fails = 0
        nmatches -= n - res.n_triangulated
        if nmatches < 0.1 * n or nmatches < 150:
            has_first = False
            return "reset_triangulated"
        r.set_second_image(im, 1.0)
        r.set_points_twoview(fl, tv)
        pose, _, good, _, _ = r.Refine(se3_data(res.R.astype(np.float64), res.t.astype(np.float64)))
        return "success"

    for img in frames:
        actions.append(one(img))
        states.append(rng.state)
        returned.append(actions[-1] == "success")
    ba = window_of(s)
    ba.insertFrame(make_frame(IDENTITY, fid=0))
    ba.set_frame_image_from(0, first_im)
    why, hd = r.seed_window(ba, 0)
    ba.makeIDX()
    o = dict(returned=returned, actions=actions, states=states, record=bytes(res), pose=pose, vid=r.videpth(), good=good,
             why=why, n_seeded=np.array([len(hd)]), fails=fails)
    o.update(window_readbacks(ba))
    for x in (ba, first_im, im, fl, tv, r, u):
        x.close()
    return o


def test_driver_matches_its_twin_and_repeats():
    frames, keys, s = sequence()
    d, t = run_driver(0), run_twin(0)
    print([(h["action"], h["nmatches"], h["mean_flow"], h["why"], hex(h["rng_state"])) for h in d["history"]])
    assert same(d["img8"], frames[0])                                # the identity undistorter: cvImgL is the raw frame
    assert t["actions"] == ["first", "stationary", "fit_failed", "success"]          # the exits the models took
    assert [h["action"] for h in d["history"]] == t["actions"]
    assert [h["rng_state"] for h in d["history"]] == t["states"]
    assert d["returned"] == t["returned"] == [False, False, False, True]
    h = d["history"]
    assert h[1]["mean_flow"] < 2 and h[1]["NumFails"] == 0 and h[2]["NumFails"] == 1 and h[3]["NumFails"] == 0
    assert h[2]["why"] in (1, 2, 3, 4) and h[3]["why"] == 0 and h[3]["nmatches"] >= 150
    assert h[0]["rng_state"] == h[1]["rng_state"] != h[2]["rng_state"] != h[3]["rng_state"]
    assert d["fails"] == t["fails"] == 0
    rec = bytearray(d["record"])
    assert bytes(rec[104:112]) == np.array(state_words(t["states"][-1]), np.uint32).tobytes()
    rec[104:112] = bytes(8)
    assert bytes(rec) == t["record"]
    keys_ = [k for k in t if k not in ("actions", "states", "record", "returned", "fails")]
    for k in keys_:
        assert same(d[k], t[k]), k
    assert d["n_seeded"][0] >= 100 and np.isfinite(d["pose"]).all() and d["good"].sum() >= 100
    # a second run from a fresh object is bit-identical
    d2 = run_driver(0)
    assert d2["history"] == d["history"] and d2["record"] == d["record"]
    for k in keys_ + ["img8"]:
        assert same(d[k], d2[k]), k


def test_driver_extracts_its_own_keys():
    """Without keys= the frame's mvKeys come from Frame::Extract's path on the device.  Two frames of
    tests/test_gpu_init.py's chain scene (a field moved by (1.5, 0.5) px, so the second frame is stationary): the
    driver's first-frame keys and its tracked state equal a twin's that calls the same bricks by hand."""
    import extract_cases as xc
    import flow_cases as fc
    from undist_cases import CASES, gamma_G, lib_calib
    from hslam_amd.extract import FeatureExtractor
    from hslam_amd.flow import KeypointFlow
    from hslam_amd.image import DeviceImage
    from hslam_amd.initializer import Initializer
    from hslam_amd.select import PixelSelector
    from hslam_amd.undistort import Undistorter
    W, H = 320, 240
    c = CASES["chain"]
    u = Undistorter(lib_calib("chain"))
    u.set_photometric(gamma_G(), None)
    f0 = fc.field(c["w_in"], c["h_in"], seed=61)
    raws = [fc.crop8(f0), fc.crop8(np.clip(fc.ndimage.shift(f0, (0.5, 1.5), order=3, mode="nearest"), 0, 255))]
    pat = xc.random_pattern()
    ini = Initializer(W, H, K4_320, 4000, pattern=pat, density=600)
    returned = [ini.Initialize(raw, u) for raw in raws]
    # the twin
    im, sel, ex, fl = DeviceImage(W, H, 4), PixelSelector(W, H), FeatureExtractor(W, H, 4000, pat), KeypointFlow(W, H, 4000)
    im.set_u8(u, raws[0])
    sel.makeMapsImage(im, 0, 600)
    n = ex.extract_image(sel, im)
    assert fl.set_first_extracted(ex) == n > 100
    im.set_u8(u, raws[1])
    sel.makeMapsImage(im, 1, 600)
    n2 = ex.extract_image(sel, im)
    nmatches = fl.track_image(im, 7)
    mean = fl.mean_flow()
    h = ini.history
    assert returned == [False, False] and h[0]["action"] == "first" and h[0]["nFeatures"] == n and h[1]["nFeatures"] == n2
    model = CvRng(0)
    model.skip(3 * n)                                                # ColorVec
    assert h[0]["rng_state"] == model.state
    assert f32(nmatches) >= f32(0.2) * f32(n) and mean < 2           # the twin's exit: stationary
    assert (h[1]["action"], h[1]["nmatches"], h[1]["rng_state"]) == ("stationary", nmatches, model.state)
    assert f32(h[1]["mean_flow"]).tobytes() == f32(mean).tobytes()
    a, b = ini.flow.get(), fl.get()
    for k in b:
        assert same(a[k], b[k]), k
    for o in (ini, im, ex, fl, u):
        o.close()


# ---- 6. lifetime

def test_new_buffers_and_the_driver_return_every_allocation():
    from hslam_amd._lib import load
    from hslam_amd.flow import KeypointFlow
    from hslam_amd.initializer import Initializer
    from hslam_amd.twoview import TwoViewFit
    lib = load()
    lib.hs_debug_live_allocations.argtypes, lib.hs_debug_live_allocations.restype = [], C.c_longlong
    frames, keys, s = sequence()
    gc.collect()
    start = lib.hs_debug_live_allocations()
    for _ in range(2):
        t = TwoViewFit(67, K4_320)
        held = lib.hs_debug_live_allocations()
        assert held > start
        t.draw(draw_status(67), 9)
        fl = seven_good_flow()
        held_fl = lib.hs_debug_live_allocations()
        assert held_fl > held
        assert t.fit_flow_drawn(fl, 9).why == 5
        fl.mean_flow_device()
        assert lib.hs_debug_live_allocations() == held_fl            # nothing is allocated after create
        fl.close()
        t.close()
        assert lib.hs_debug_live_allocations() == start
    u = identity_undistorter(s)
    base = lib.hs_debug_live_allocations()
    ini = Initializer(s.width, s.height, s.K4, 300)
    held = lib.hs_debug_live_allocations()
    assert not ini.Initialize(frames[0], u, 1.0, keys=keys) and not ini.Initialize(frames[1], u, 1.0, keys=keys)
    assert [h["action"] for h in ini.history] == ["first", "stationary"]
    assert lib.hs_debug_live_allocations() >= held                   # the image and refiner bricks stage at first use
    ini.close()
    assert lib.hs_debug_live_allocations() == base
    u.close()
    assert lib.hs_debug_live_allocations() == start
