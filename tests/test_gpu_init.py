"""include/hs_init.h on the device: the refiner's frames from a device image, its points from the flow context's
first-frame keys, and System::InitFromInitializer's point loop staged into a BA window.  Bar: bit-identity with the host
entries they replace (hs_image_get + hs_refiner_set_frames, hs_refiner_set_points, and the host loop videpth read-back
-> hs_tracer_add_points at +0.5 -> hs_ba_insert_points + hs_ba_set_last_residuals); expected values never come from
the new entries."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K_OF = {(160, 120): np.array([[64.0, 0, 79.5], [0, 63.6, 59.5], [0, 0, 1.0]]),
        (320, 240): np.array([[128.0, 0, 159.5], [0, 127.2, 119.5], [0, 0, 1.0]])}
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def scene(n, w=160, h=120, exposures=(1.0, 1.0)):
    from hslam_amd.scene import make_refine_scene
    s = make_refine_scene(n, width=w, height=h, K=K_OF[(w, h)], tri_frac=0.6, exposures=exposures)
    assert len(s.u) == n and s.tri.sum() >= 3 and (s.tri == 0).sum() >= 1
    return s


def fimgs(s):
    """fImgL of the two frames (the intensity lane of the scene's DirPyr[0])."""
    return [np.ascontiguousarray(s.img1[..., 0]), np.ascontiguousarray(s.img2[..., 0])]


def device_images(s):
    from hslam_amd.image import DeviceImage
    out = []
    for f in fimgs(s):
        im = DeviceImage(s.width, s.height, 1)
        im.set_raw(f)
        out.append(im)
    return out


def bare(s):
    from hslam_amd.refine import DirectRefinement
    return DirectRefinement.bare(s.width, s.height, s.K4)


def ctor_videpth(s):
    """Initializer.cpp:155-159: 1.0 / z in double, stored as float; -1 where not triangulated."""
    return np.where(s.tri == 1, (1.0 / s.z.astype(np.float64)).astype(np.float32), np.float32(-1.0)).astype(np.float32)


def refiner_outputs(r, s, refine=True):
    o = {}
    H, b, Hs, bs, res = r.calcResAndGS(s.T_init)
    o.update(H=H, b=b, Hsc=Hs, bsc=bs, res=res)
    o.update({"p0." + k: v for k, v in r.points().items()})
    if refine:
        pose, vid, good, it, sn = r.Refine(s.T_init, videpth=ctor_videpth(s))
        o.update(pose=pose, vid=vid, good=good, it=np.array([it, int(sn)]), log=r.log())
        o.update({"p1." + k: v for k, v in r.points().items()})
    return o


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert same(a[k], b[k]), k


# ---- 1. the two frames from device images

def test_frames_from_device_images_match_set_frames():
    s = scene(300, exposures=(1.0, 1.3))
    im1, im2 = device_images(s)
    a, b = bare(s), bare(s)
    a.set_first_image(im1, s.expo1)
    a.set_second_image(im2, s.expo2)
    b.set_frames(im1.get(0)[0], im2.get(0)[0], s.expo1, s.expo2)
    for r in (a, b):
        r.set_points(s.u, s.v, s.tri, s.z)
    oa, ob = refiner_outputs(a, s), refiner_outputs(b, s)
    assert_same(oa, ob)
    assert ob["it"][0] >= 2 and ob["good"].sum() >= 10 and np.isfinite(ob["res"]).all() and ob["res"][2] > 0

    # one image object for both frames, overwritten right after each hand-off with no wait in between
    c = bare(s)
    f1, f2 = fimgs(s)
    im = im1
    im.set_raw(f1)
    c.set_first_image(im, s.expo1)
    im.set_raw(f2)
    c.set_second_image(im, s.expo2)
    im.set_raw(np.ascontiguousarray(f1[::-1]))
    c.set_points(s.u, s.v, s.tri, s.z)
    assert_same(refiner_outputs(c, s), ob)
    for o in (a, b, c, im1, im2):
        o.close()


def test_frames_are_set_independently():
    """haveFrames is "both set": one image alone does not make the refiner ready, either order does."""
    from hslam_amd._lib import HsError
    s = scene(33)
    im1, im2 = device_images(s)
    want = None
    for order in ((0, 1), (1, 0)):
        r = bare(s)
        r.set_points(s.u, s.v, s.tri, s.z)
        for k, which in enumerate(order):
            if k == 1:
                with pytest.raises(HsError, match=r"\(-5\)"):
                    r.calcResAndGS(s.T_init)
            (r.set_first_image if which == 0 else r.set_second_image)(im1 if which == 0 else im2, 1.0)
        got = refiner_outputs(r, s, refine=False)
        if want is None:
            want = got
        assert_same(got, want)
        r.close()
    im1.close()
    im2.close()


# ---- 2. the points from the flow context

def img8_of(f):
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("n", [7, 33, 300])
def test_points_from_flow_match_set_points(n):
    from hslam_amd.flow import KeypointFlow
    s = scene(n)
    f1, f2 = fimgs(s)
    xy = np.stack([s.u, s.v], 1).astype(np.float32)
    fl = KeypointFlow(s.width, s.height, n)
    fl.set_first(img8_of(f1), xy)
    fl.track(img8_of(f2), 7)
    g = fl.get()
    assert same(g["first_xy"], xy) and np.any(g["xy"] != xy)         # MatchedPts has moved; FirstFramePts has not
    a, b = bare(s), bare(s)
    for r in (a, b):
        r.set_frames(s.img1, s.img2, s.expo1, s.expo2)
    a.set_points_flow(fl, s.tri, s.z)
    b.set_points(s.u, s.v, s.tri, s.z)
    pa, pb = a.points(), b.points()
    assert_same(pa, pb)
    assert same(a.videpth(), b.videpth()) and same(b.videpth(), ctor_videpth(s))
    assert_same(refiner_outputs(a, s, refine=False), refiner_outputs(b, s, refine=False))
    for o in (a, b, fl):
        o.close()


def test_points_from_flow_refuse_a_key_outside_the_image():
    from hslam_amd._lib import HsError
    from hslam_amd.flow import KeypointFlow
    s = scene(33)
    f1, _ = fimgs(s)
    xy = np.stack([s.u, s.v], 1).astype(np.float32)
    xy[20, 0] = s.width - 0.5                                        # > W - 1
    fl = KeypointFlow(s.width, s.height, 33)
    fl.set_first(img8_of(f1), xy)
    r = bare(s)
    r.set_frames(s.img1, s.img2)
    r.set_points(s.u, s.v, s.tri, s.z)                               # points it held before
    with pytest.raises(HsError, match=r"\(-1\).*outside"):
        r.set_points_flow(fl, s.tri, s.z)
    r.n = 33
    with pytest.raises(HsError, match=r"\(-5\).*no points"):
        r.points()
    with pytest.raises(HsError, match=r"\(-5\)"):
        r.calcResAndGS(s.T_init)
    # before a first frame, and a flow of another size
    empty = KeypointFlow(s.width, s.height, 33)
    with pytest.raises(HsError, match=r"\(-5\).*first"):
        r.set_points_flow(empty, s.tri, s.z)
    wide = KeypointFlow(s.width + 32, s.height, 33)
    wide.set_first(np.zeros((s.height, s.width + 32), np.uint8), xy)
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        r.set_points_flow(wide, s.tri, s.z)
    for o in (r, fl, empty, wide):
        o.close()


# ---- 3. seeding the first window

def new_window(s, capacity):
    from hslam_amd.ba import BAWindow, make_frame
    ba = BAWindow(camera=(s.width, s.height, 1, s.K), capacity=capacity)
    ba.insertFrame(make_frame(IDENTITY, fid=0))
    return ba


def border_ok(x, y, w, h):
    return (x >= 2) & (y >= 2) & (x < w - 3) & (y < h - 3)


def host_seed(r, ba, s, dirpyr0):
    """InitFromInitializer's loop decided on the host: videpth read back, the ImmaturePoint constructor through a
    tracer, the survivors pushed up again.  Returns (why, handles)."""
    from hslam_amd.trace import ImmatureTracer
    vid = r.videpth()
    x, y = s.u.astype(np.float32) + np.float32(0.5), s.v.astype(np.float32) + np.float32(0.5)
    n = len(vid)
    why = np.zeros(n, np.uint8)
    why[vid <= 0] = 1                                                # System.cpp:267
    why[(why == 0) & ~border_ok(x, y, s.width, s.height)] = 3        # the documented deviation
    cand = np.nonzero(why == 0)[0]
    tr = ImmatureTracer(s.width, s.height, max(1, len(cand)))
    tr.set_host_image(0, dirpyr0)
    tr.add_points(np.zeros(len(cand), np.int32), x[cand], y[cand])
    p = tr.points()
    fin = np.isfinite(p["energyTH"])                                 # :273
    why[cand[~fin]] = 2
    keep = cand[fin]
    hd = ba.insertPoints(np.zeros(len(keep), np.int32), x[keep], y[keep], vid[keep], vid[keep], p["color"][fin],
                         p["weights"][fin], has_prior=np.ones(len(keep), np.uint8))
    # the reference's lastResiduals pairs are value-initialised: (nullptr, ResState::IN)
    ba.setLastResiduals(hd, -np.ones((len(keep), 2), np.int32), np.zeros((len(keep), 2), np.uint8))
    tr.close()
    return why, hd


def window_readbacks(ba):
    st, ps, lr = ba.structure(), ba.point_state(), ba.lastResiduals()
    o = {"st." + k: v for k, v in st.items() if k != "handles"}
    o.update({"ps." + k: v for k, v in ps.items()})
    o.update({"last." + k: v for k, v in lr.items()})
    return o


def second_frame_readbacks(ba, pose, image=None, host_image=None):
    from hslam_amd.ba import make_frame
    ba.insertFrame(make_frame(pose, fid=1), image=host_image)
    if image is not None:
        ba.set_frame_image_from(1, image)
    n_added = ba.addResidualsToNewest()
    o = {"n_added": np.array([n_added]), "E": np.array([ba.linearizeAll(reset=True)])}
    for which in (0, 2):
        H, b = ba.system(which)
        o[f"H{which}"], o[f"b{which}"] = H, b
    o.update({"res0." + k: v for k, v in ba.residuals().items()})
    o["opt"] = ba.optimize(3)[1]
    o.update({"res." + k: v for k, v in ba.residuals().items()})
    o.update({"ps." + k: v for k, v in ba.point_state().items()})
    o.update({"last." + k: v for k, v in ba.lastResiduals().items()})
    return o


def seeded_pair(s, refine, capacity):
    """(refiner, device-seeded window, why, handles), (host-seeded window, why, handles), pose, images"""
    im1, im2 = device_images(s)
    r = bare(s)
    r.set_first_image(im1, s.expo1)
    r.set_second_image(im2, s.expo2)
    r.set_points(s.u, s.v, s.tri, s.z)
    pose = np.array(s.T_init, np.float64)
    if refine:
        pose, vid, good, _, _ = r.Refine(s.T_init, videpth=ctor_videpth(s))
        assert same(r.videpth(), vid)                                # the write-back applied to the constructor's array
        assert len(vid) < 300 or np.any(vid != ctor_videpth(s))      # the refinement moved some depth
    else:
        assert same(r.videpth(), ctor_videpth(s))
    bd, bh = new_window(s, capacity), new_window(s, capacity)
    bd.set_frame_image_from(0, im1)
    bh.set_frame_image_from(0, im1)
    why_d, hd_d = r.seed_window(bd, 0)
    why_h, hd_h = host_seed(r, bh, s, im1.get(0)[0])
    return r, (bd, why_d, hd_d), (bh, why_h, hd_h), pose, (im1, im2)


@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("n, w, h", [(7, 160, 120), (300, 160, 120), (1100, 320, 240)])
def test_seeded_window_matches_the_host_path(n, w, h, refine):
    s = scene(n, w, h)
    r, (bd, why_d, hd_d), (bh, why_h, hd_h), pose, (im1, im2) = seeded_pair(s, refine, capacity=n + 8)
    assert same(why_d, why_h)
    assert len(hd_d) == len(hd_h) == int((why_h == 0).sum()) >= 3
    if n > 1024:
        assert (why_h[:1024] == 0).sum() >= 100 and (why_h[1024:] == 0).sum() >= 10   # both sweeps seed
    assert np.all(np.diff(hd_d) == 1) and same(hd_d - hd_d[0], hd_h - hd_h[0])
    a, b = window_readbacks(bd), window_readbacks(bh)
    assert_same(a, b)
    assert len(a["ps.idepth"]) == len(hd_h)
    assert same(a["ps.idepth"], r.videpth()[why_h == 0])            # mvKeys order
    assert not a["last.state"].any() and np.all(a["last.target"] == -1)             # (none, IN) twice
    a2 = second_frame_readbacks(bd, pose, image=im2)
    b2 = second_frame_readbacks(bh, pose, image=im2)
    assert_same(a2, b2)
    assert b2["n_added"][0] == len(hd_h) and np.isfinite(b2["E"][0]) and b2["E"][0] > 0 and len(b2["opt"]) >= 2
    assert np.any(b2["H0"] != 0)
    for o in (r, bd, bh, im1, im2):
        o.close()


def test_every_skip_rule_without_a_refine():
    from hslam_amd.refine import DirectRefinement
    s0 = scene(300)
    w, h = s0.width, s0.height
    im1, _ = device_images(s0)
    dirpyr0 = im1.get(0)[0].copy()
    u, v, tri, z = s0.u.copy(), s0.v.copy(), s0.tri.copy(), s0.z.copy()
    t = np.nonzero(tri == 1)[0]
    i_neg, i_nan, i_edge = t[1], t[len(t) // 2], t[-2]
    z[i_neg] = -2.0                                                  # triangulated behind the camera
    u[i_edge] = w - 3                                                # u + 0.5 >= W - 3
    py, px = int(v[i_nan] + 0.5), int(u[i_nan] + 0.5)                # the texel under the pattern's centre tap
    dirpyr0[py, px, 0] = np.nan

    class S:                                                         # the scene with these edits
        width, height, K = w, h, s0.K
    S.u, S.v, S.tri, S.z = u, v, tri, z
    r = DirectRefinement.bare(w, h, s0.K4)
    r.set_frames(dirpyr0, s0.img2)
    r.set_points(u, v, tri, z)
    # the numpy rule
    vid = np.where(tri == 1, (1.0 / z.astype(np.float64)).astype(np.float32), np.float32(-1)).astype(np.float32)
    assert same(r.videpth(), vid)
    x, y = u.astype(np.float32) + np.float32(0.5), v.astype(np.float32) + np.float32(0.5)
    want = np.zeros(300, np.uint8)
    want[vid <= 0] = 1
    want[(want == 0) & ~border_ok(x, y, w, h)] = 3
    pat = [(0, -2), (-1, -1), (1, -1), (-2, 0), (0, 0), (2, 0), (-1, 1), (0, 2)]
    for i in np.nonzero(want == 0)[0]:
        taps = [dirpyr0[int(y[i] + dy) + oy, int(x[i] + dx) + ox, 0] for dx, dy in pat for oy in (0, 1) for ox in (0, 1)]
        if not np.isfinite(taps).all():
            want[i] = 2
    assert want[i_neg] == 1 and want[i_nan] == 2 and want[i_edge] == 3 and (want[tri == 0] == 1).all()
    bd, bh = new_window(S, 300), new_window(S, 300)
    why, hd = r.seed_window(bd, 0)
    assert same(why, want)
    for code in range(4):
        assert (why == code).sum() == (want == code).sum() >= 1, code
    why_h, hd_h = host_seed(r, bh, S, dirpyr0)
    assert same(why_h, want)
    a, b = window_readbacks(bd), window_readbacks(bh)
    assert_same(a, b)
    assert np.all(np.diff(hd) == 1) and same(a["ps.idepth"], vid[want == 0])        # the seeded keep mvKeys order
    for o in (r, bd, bh, im1):
        o.close()


# ---- 4. errors and lifetime

def test_errors_leave_both_objects_unchanged_and_nothing_leaks():
    from hslam_amd._lib import HsError, load
    from hslam_amd.ba import BAWindow, make_frame
    from hslam_amd.image import DeviceImage
    lib = load()
    lib.hs_debug_live_allocations.argtypes, lib.hs_debug_live_allocations.restype = [], C.c_longlong
    s = scene(300)
    gc.collect()
    start = lib.hs_debug_live_allocations()
    im1, im2 = device_images(s)
    r = bare(s)
    empty = DeviceImage(s.width, s.height, 1)
    wide = DeviceImage(s.width + 32, s.height, 1)
    wide.set_raw(np.zeros((s.height, s.width + 32), np.float32))
    with pytest.raises(HsError, match=r"\(-5\).*no frame"):
        r.set_first_image(empty)
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        r.set_second_image(wide)
    r.set_first_image(im1)
    ba = new_window(s, 400)
    with pytest.raises(HsError, match=r"\(-5\).*no points"):         # seeding before set_points
        r.seed_window(ba, 0)
    r.set_points(s.u, s.v, s.tri, s.z)
    with pytest.raises(HsError, match=r"\(-5\)"):                    # a failed set left no second frame behind
        r.calcResAndGS(s.T_init)
    r.set_second_image(im2)
    before = refiner_outputs(r, s, refine=False)
    with pytest.raises(HsError, match=r"\(-1\).*frame"):             # not a window frame
        r.seed_window(ba, 1)
    with pytest.raises(HsError, match=r"\(-1\).*frame"):
        r.seed_window(ba, -1)
    other = BAWindow(camera=(s.width + 32, s.height, 1, s.K), capacity=400)
    other.insertFrame(make_frame(IDENTITY, fid=0))
    with pytest.raises(HsError, match=r"\(-1\).*size"):
        r.seed_window(other, 0)
    small = new_window(s, 5)
    with pytest.raises(HsError, match=r"\(-6\)"):                    # nothing staged: the window is unchanged
        r.seed_window(small, 0)
    five = np.full(5, 20.0, np.float32)
    small.insertPoints(np.zeros(5, np.int32), five, five, five, five, np.ones((5, 8)), np.ones((5, 8)))
    small.makeIDX()
    assert small.n_points == 5 and small.nF == 1                     # its whole capacity was still free
    why, hd = r.seed_window(ba, 0)                                   # more capacity: the same call works, and none of
    ba.makeIDX()                                                     # the failures above left a point in this window
    assert ba.n_points == len(hd) == int((why == 0).sum()) > 5
    assert_same(refiner_outputs(r, s, refine=False), before)
    for o in (r, ba, other, small, im1, im2, empty, wide):
        o.close()
    gc.collect()
    assert lib.hs_debug_live_allocations() == start


# ---- 5. the whole chain on the device against the same chain through the host entries

def test_initializer_chain_matches_the_host_entries():
    import extract_cases as xc
    import flow_cases as fc
    from undist_cases import CASES, gamma_G, lib_calib
    from hslam_amd.extract import FeatureExtractor
    from hslam_amd.flow import KeypointFlow
    from hslam_amd.image import DeviceImage
    from hslam_amd.pyr import dir_pyramid
    from hslam_amd.refine import DirectRefinement
    from hslam_amd.select import PixelSelector
    from hslam_amd.undistort import Undistorter
    W, H, LEVELS = 320, 240, 4                                       # tests/test_gpu_image.py's consumer scene
    K = K_OF[(W, H)]
    K4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    c = CASES["chain"]
    u = Undistorter(lib_calib("chain"))
    u.set_photometric(gamma_G(), None)
    f0 = fc.field(c["w_in"], c["h_in"], seed=61)
    raws = [fc.crop8(f0), fc.crop8(np.clip(fc.ndimage.shift(f0, (0.5, 1.5), order=3, mode="nearest"), 0, 255))]
    pat = xc.random_pattern()

    class S:
        width, height = W, H
    S.K = K

    def two_view(xy):
        """tri / z a two-view fit would return for a fronto-parallel scene 2 m away moved by (1.5, 0.5) px, and its
        pose; every fifth key not triangulated, the depth rippled so the idepths differ."""
        n = len(xy)
        tri = (np.arange(n) % 5 != 0).astype(np.uint8)
        z = (2.0 * (1.0 + 0.05 * np.sin(0.05 * xy[:, 0]) * np.cos(0.07 * xy[:, 1]))).astype(np.float32)
        pose = np.array([0, 0, 0, 1, 2.0 * 1.5 / K[0, 0], 2.0 * 0.5 / K[1, 1], 0.0])
        return tri, z, pose

    def finish(r, ba, seed):
        xy = S.xy
        tri, z, pose0 = two_view(xy)
        pose, vid, good, it, sn = r.Refine(pose0, videpth=np.where(tri == 1, (1.0 / z.astype(np.float64)).astype(
            np.float32), np.float32(-1)).astype(np.float32))
        why, hd = seed(r, ba)
        o = dict(pose=pose, vid=vid, good=good, it=np.array([it, int(sn)]), log=r.log(), why=why, nh=np.array([len(hd)]))
        o.update(window_readbacks(ba))
        return o, pose

    # the device chain: one image object, every hand-off device to device
    im = DeviceImage(W, H, LEVELS)
    sel, ex, fl = PixelSelector(W, H), FeatureExtractor(W, H, 4000, pat), KeypointFlow(W, H, 4000)
    r = DirectRefinement.bare(W, H, K4)
    ba = new_window(S, 4000)
    im.set_u8(u, raws[0])
    sel.makeMapsImage(im, 0, 600)
    n = ex.extract_image(sel, im)
    assert fl.set_first_extracted(ex) == n >= 100
    r.set_first_image(im, 1.0)
    ba.set_frame_image_from(0, im)
    im.set_u8(u, raws[1])
    fl.track_image(im, 7)
    r.set_second_image(im, 1.0)
    S.xy = fl.get()["first_xy"]
    S.u, S.v = S.xy[:, 0].copy(), S.xy[:, 1].copy()
    tri, z, _ = two_view(S.xy)
    S.tri, S.z = tri, z
    r.set_points_flow(fl, tri, z)
    od, pose_d = finish(r, ba, lambda r_, ba_: r_.seed_window(ba_, 0))
    od2 = second_frame_readbacks(ba, pose_d, image=im)
    flow_d = fl.get()

    # the same chain through the host entries
    fimg, img8 = zip(*[u.undistort(raw) for raw in raws])
    dp = [dir_pyramid(f, 1)[0][0] for f in fimg]
    sel2, ex2, fl2 = PixelSelector(W, H), FeatureExtractor(W, H, 4000, pat), KeypointFlow(W, H, 4000)
    sel2.makeMapsRaw(fimg[0], 0, 600)
    assert ex2.extract_u8(sel2, u, raws[0]) == n
    keys = ex2.get()["xy"]
    assert same(keys, S.xy)
    fl2.set_first(img8[0], keys)
    fl2.track(img8[1], 7)
    r2 = DirectRefinement.bare(W, H, K4)
    r2.set_frames(dp[0], dp[1], 1.0, 1.0)
    r2.set_points(keys[:, 0], keys[:, 1], tri, z)
    from hslam_amd.ba import BAWindow, make_frame
    ba2 = BAWindow(camera=(W, H, 1, K), capacity=4000)
    ba2.insertFrame(make_frame(IDENTITY, fid=0), image=dp[0])
    oh, pose_h = finish(r2, ba2, lambda r_, ba_: host_seed(r_, ba_, S, dp[0]))
    oh2 = second_frame_readbacks(ba2, pose_h, host_image=dp[1])
    assert_same(od, oh)
    assert_same(od2, oh2)
    fh = fl2.get()
    for k in fh:
        assert same(flow_d[k], fh[k]), k
    assert oh["nh"][0] >= 50 and (oh["why"] == 1).sum() >= n // 5 and oh2["E"][0] > 0
    for o in (im, ex, fl, r, ba, ex2, fl2, r2, ba2, u):
        o.close()
