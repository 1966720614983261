"""include/hs_twoview.h on the device against its numpy model (tests/twoview_ref.py), layer by layer: the scoring on
given matrices, the hypothesis matrices, CheckRT on given motions, the whole fit, determinism, the hand-off from the
flow context and into the refiner, the refusals and the lifetime.  Expected values never come from the device.

Bars.  Scores and masks: equality.  Hypothesis matrices: 4 x the model's own spread (two fp64 routes to the same
matrix, measured here on the CPU by tests/test_twoview.py's model_spread) with a floor of 2^-22 for the two fp32
roundings.  p3d, R, t, the median depth: 4 x the largest relative distance between the model's fp64 x3D and its fp32
rounding (2^-24 at most, so 2^-22 at most)."""
import ctypes as C
import functools
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import twoview_cases as tc  # noqa: E402
import twoview_ref as tr  # noqa: E402
from test_twoview import canon, model_spread  # noqa: E402
from hslam_amd.twoview import TwoViewFit  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32

# n: one possible set; < 51 good matches; no multiple of 64; the block tail; more than one pass of every strided loop
FIT_CASES = [("general", 8, 1), ("general", 40, 3), ("general", 67, 200), ("general", 300, 200), ("general", 2049, 200),
             ("planar", 67, 3), ("planar", 300, 200), ("planar", 2049, 3), ("rotation", 300, 200),
             ("outlier", 300, 200), ("degenerate", 300, 200)]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def ref_fit(kind, n, ns):
    s = tc.scene(kind, n)
    return tr.fit(s["xy1"], s["xy2"], s["status"], tc.sets_of(kind, n, ns), tc.K4)


def device_fit(kind, n, ns, tv=None):
    s = tc.scene(kind, n)
    tv = tv or TwoViewFit(max(n, 8), tc.K4)
    res = tv.fit(s["xy1"], s["xy2"], s["status"], tc.sets_of(kind, n, ns))
    return tv, res


def p3d_bar(o):
    """4 x the model's own fp64-against-fp32 spread of x3D, relative."""
    worst = 0.0
    for r in o["rt"]:
        m = r["passed"] != 0
        if m.any():
            x64, x32 = r["p3d64"][m], r["p3d"][m].astype(np.float64)
            worst = max(worst, float((np.abs(x64 - x32) / np.abs(x64)).max()))
    assert worst <= 2.0 ** -24
    return 4 * worst


def perturbed(M, px, rng):
    """The homography / fundamental matrix moved so that points shift by about `px` pixels."""
    M = np.asarray(M, np.float64)
    d = rng.normal(size=M.shape)
    d[..., 2, :] = 0
    scale = np.abs(M[..., :2, 2]).max(axis=-1)[..., None, None] + 1.0
    return (M + d * px * 1e-3 * scale * np.array([[1e-1, 1e-1, 1.0]] * 3)).astype(f32)


# ---- 1. the scoring on caller-supplied matrices

@pytest.mark.parametrize("kind, n", [("general", 300), ("planar", 2049), ("general", 67)])
def test_score_models_matches_the_model(kind, n):
    s = tc.scene(kind, n)
    o = ref_fit(kind, n, 200 if n != 2049 else 3)
    tv, _ = device_fit(kind, n, 200 if n != 2049 else 3)
    rng = np.random.default_rng(9)
    H21, F21 = o["H21"][:30], o["F21"][:30]
    for px in (0.0, 1.0, 3.0):
        h = H21 if px == 0 else perturbed(H21, px, rng)
        f = F21 if px == 0 else perturbed(F21, px, rng)
        hi = o["H12"][:30] if px == 0 else tr.inv3(h.astype(np.float64)).astype(f32)
        want = tr.score_models(h, hi, f[:17], s["xy1"], s["xy2"], s["status"])
        tv.score_models(h, hi, f[:17])                       # n_h != n_f
        g = tv.get()
        for k in ("scores_h", "scores_f", "inliers_h", "inliers_f"):
            assert np.array_equal(g[k], want[k]), (k, px)
        assert 0 < want["inliers_h"].sum() + want["inliers_f"].sum() < 2 * n
        assert np.isfinite(want["scores_h"]).all()
    tv.close()


# ---- 2. the hypothesis matrices

@pytest.mark.parametrize("kind, n, ns", [c for c in FIT_CASES if c[0] in ("general", "planar") and c[1] >= 67])
def test_hypothesis_matrices_within_the_models_spread(kind, n, ns):
    o = ref_fit(kind, n, ns)
    tv, _ = device_fit(kind, n, ns)
    g = tv.get()
    spread, def_h, def_f = model_spread(kind, n, ns)
    bar = max(4 * spread, 2.0 ** -22)
    assert (~def_h).mean() <= 0.05 and (~def_f).mean() <= 0.05
    dh = np.abs(canon(g["models_h"]) - canon(o["H21"], g["models_h"])).max(axis=1)
    df = np.abs(canon(g["models_f"]) - canon(o["F21"], g["models_f"])).max(axis=1)
    print(f"{kind} n={n}: H {dh[def_h].max():.3e} F {df[def_f].max():.3e} bar {bar:.3e}")
    assert dh[def_h].max() <= bar and df[def_f].max() <= bar
    tv.close()


# ---- 3. CheckRT on caller-supplied motions

@pytest.mark.parametrize("kind, n, ns", [("general", 300, 200), ("planar", 300, 200), ("general", 2049, 200),
                                         ("general", 40, 3)])
def test_check_rt_matches_the_model(kind, n, ns):
    s = tc.scene(kind, n)
    o = ref_fit(kind, n, ns)
    assert o["n_rt"] in (4, 8)
    inl = o["inliers_f"] if o["model"] else o["inliers_h"]
    tv, _ = device_fit(kind, n, ns)
    tv.check_rt(o["R_all"], o["t_all"], inl)
    g = tv.get_rt()
    bar = p3d_bar(o)
    assert len(g["n_good"]) == o["n_rt"]
    flagged = 0
    for h, r in enumerate(o["rt"]):
        clear = ~r["amb"]
        flagged += int((r["amb"] & (inl != 0)).sum())
        assert np.array_equal(g["good"][h][clear], r["good"][clear]), h
        assert np.array_equal(g["passed"][h][clear], r["passed"][clear]), h
        both = (g["passed"][h] != 0) & (r["passed"] != 0)
        err = np.abs(g["p3d"][h][both].astype(np.float64) - r["p3d"][both]) / np.abs(r["p3d64"][both])
        assert err.size == 0 or err.max() <= bar, (h, float(err.max()), bar)
        if np.array_equal(g["passed"][h], r["passed"]):
            assert g["n_good"][h] == r["n_good"]
            if np.array_equal(g["cos_parallax"][h], r["cos"]):
                assert g["parallax"][h] == r["parallax"], h
            else:
                assert abs(g["parallax"][h] - r["parallax"]) <= bar * max(1.0, abs(r["parallax"])) * 180 / np.pi
        else:
            assert abs(int(g["n_good"][h]) - r["n_good"]) <= int(r["amb"].sum())
    assert flagged <= 0.01 * o["n_rt"] * max(int((inl != 0).sum()), 1)
    tv.close()


# ---- 4. the whole fit

@pytest.mark.parametrize("kind, n, ns", FIT_CASES)
def test_fit_matches_the_model(kind, n, ns):
    o = ref_fit(kind, n, ns)
    # a property of the chosen cases, asserted on the model: the winners are clear
    if o["best_h"] >= 0:
        assert o["margin_h"] > 1e-4
    if o["best_f"] >= 0:
        assert o["margin_f"] > 1e-4
    tv, res = device_fit(kind, n, ns)
    g = tv.get()
    for k in ("ok", "why", "model", "best_h", "best_f", "best_rt", "n_rt"):
        assert getattr(res, k) == o[k], (k, getattr(res, k), o[k])
    # the scores are equal where the fp32 matrices are (test_score_models_*); here a matrix may differ in its last
    # bit, and 1e-4 is the distance at which device and model could disagree on a winner asserted clear by 1e-4
    assert abs(res.SH - o["SH"]) <= 1e-4 * o["SH"] and abs(res.SF - o["SF"]) <= 1e-4 * o["SF"]
    print(f"{kind} n={n}: scores equal H {np.array_equal(g['scores_h'], o['scores_h'])} "
          f"F {np.array_equal(g['scores_f'], o['scores_f'])}, models equal H {np.array_equal(g['models_h'], o['H21'])} "
          f"F {np.array_equal(g['models_f'], o['F21'])}")
    for m in ("h", "f"):
        clear = ~o["amb_" + m]
        assert np.array_equal(g["inliers_" + m][clear], o["inliers_" + m][clear]), m
        assert o["amb_" + m].mean() <= 0.01
    clear = ~o["amb_rt"]
    assert np.array_equal(g["triangulated"][clear], o["triangulated"][clear])
    if not o["ok"]:
        assert res.ok == 0 and not g["triangulated"].any() and not res.R.any() and not res.t.any()
    assert np.isfinite(res.R).all() and np.isfinite(res.t).all() and np.isfinite(g["p3d"]).all()
    if o["ok"]:
        bar = p3d_bar(o)
        assert np.abs(res.R - o["R"]).max() <= bar
        assert np.abs(res.t - o["t"]).max() <= bar * np.abs(o["t"]).max()
        assert abs(res.median_depth - o["median_depth"]) <= bar * o["median_depth"]
        both = (g["triangulated"] != 0) & (o["triangulated"] != 0)
        z, zr = g["p3d"][both, 2].astype(np.float64), o["p3d"][both, 2].astype(np.float64)
        assert np.abs(z - zr).max() <= 2 * bar * np.abs(zr).max()          # two roundings: x3D, then / median
        if not o["amb_rt"].any():
            assert res.n_good == o["n_good"] and res.n_triangulated == o["n_triangulated"]
            assert res.parallax_deg == o["parallax"] and res.n_inliers == o["n_inliers"]
    tv.close()


def test_expected_routes():
    """The table of the cases: F for the general scene, H for the planar one, refusals for the rest."""
    for kind, n, ns, model, ok in (("general", 300, 200, 1, 1), ("general", 2049, 200, 1, 1), ("planar", 2049, 3, 0, 1)):
        tv, res = device_fit(kind, n, ns)
        assert (res.model, res.ok) == (model, ok), kind
        s = tc.scene(kind, n)
        assert tc.rotation_angle(res.R, s["R"]) < 0.05 and tc.direction_error(res.t, s["t"]) < 0.05
        assert res.n_triangulated >= 150 and res.median_depth > 0
        g = tv.get()
        assert not g["triangulated"][s["status"] == 0].any()
        z = g["p3d"][g["triangulated"] != 0, 2]
        assert np.sort(z)[(len(z) - 1) // 2] == f32(1.0)
        tv.close()
    for kind, whys in (("rotation", (3, 4)), ("outlier", (3, 4)), ("degenerate", (1, 2, 3, 4))):
        tv, res = device_fit(kind, 300, 200)
        assert res.ok == 0 and res.why in whys, (kind, res.why)
        tv.close()


# ---- 5. determinism

def test_two_fits_are_bit_identical():
    tv, a = device_fit("general", 2049, 200)
    ga, ra = tv.get(), tv.get_rt()
    other = TwoViewFit(4096, tc.K4)                                 # another context, another capacity
    _, x = device_fit("planar", 300, 200, other)                    # something else in between
    _, b = device_fit("general", 2049, 200, other)
    gb, rb = other.get(), other.get_rt()
    _, c = device_fit("general", 2049, 200, tv)
    gc_, rc = tv.get(), tv.get_rt()
    assert a.ok == 1 and bytes(a) == bytes(b) == bytes(c)
    for k in ga:
        assert same(ga[k], gb[k]) and same(ga[k], gc_[k]), k
    for k in ra:
        assert same(ra[k], rb[k]) and same(ra[k], rc[k]), k
    tv.close()
    other.close()


# ---- 6. the hand-off: from the flow context, into the refiner

K320 = np.array([[128.0, 0, 159.5], [0, 127.2, 119.5], [0, 0, 1.0]])


@functools.lru_cache(maxsize=None)
def pair_scene(trans):
    """Two rendered frames of the textured-plane world, 320 x 240, 300 keys.  With a 0.25 m baseline the tracked keys
    give a fit that succeeds by a wide margin on the F route (the model, on the flow model's tracks: 237 good against 2,
    4.7 degrees); with the 0.15 m default the reference refuses it (why 3)."""
    from hslam_amd.scene import make_refine_scene
    return make_refine_scene(300, width=320, height=240, K=K320, tri_frac=0.6, trans=trans)


def tracked_flow(trans=0.25):
    from hslam_amd.flow import KeypointFlow
    from test_gpu_init import fimgs, img8_of
    s = pair_scene(trans)
    f1, f2 = fimgs(s)
    xy = np.stack([s.u, s.v], 1).astype(f32)
    fl = KeypointFlow(s.width, s.height, 300)
    fl.set_first(img8_of(f1), xy)
    fl.track(img8_of(f2), 7)
    return s, fl


def sets_for(good, n_sets=100, seed=0):
    from hslam_amd.twoview import draw_sets
    return draw_sets(n_sets, good, np.random.default_rng(seed))


def test_fit_flow_is_fit_on_the_flows_arrays():
    s, fl = tracked_flow()
    g = fl.get()
    assert g["good"].sum() >= 8 and (g["good"] == 0).any()
    sets = sets_for(g["good"])
    a, b = TwoViewFit(300, s.K4), TwoViewFit(512, s.K4)
    ra = a.fit_flow(fl, sets)
    rb = b.fit(g["first_xy"], g["xy"], g["good"], sets)
    assert bytes(ra) == bytes(rb)
    ga, gb = a.get(), b.get()
    for k in ga:
        assert same(ga[k], gb[k]), k
    ta, tb = a.get_rt(), b.get_rt()
    for k in ta:
        assert same(ta[k], tb[k]), k
    # and the model agrees on what was fitted: a fit that succeeds on the F route
    o = tr.fit(g["first_xy"], g["xy"], g["good"], sets, s.K4)
    assert o["ok"] == 1 and o["model"] == 1 and o["margin_f"] > 1e-4
    assert (ra.ok, ra.model, ra.best_h, ra.best_f, ra.why, ra.best_rt) == (1, 1, o["best_h"], o["best_f"], 0, o["best_rt"])
    for o_ in (a, b, fl):
        o_.close()


def test_set_points_twoview_is_set_points_flow_on_the_read_back():
    from hslam_amd.refine import DirectRefinement
    from test_gpu_init import assert_same, refiner_outputs
    s, fl = tracked_flow()
    sets = sets_for(fl.get()["good"])
    tv = TwoViewFit(300, s.K4)
    res = tv.fit_flow(fl, sets)
    assert res.ok == 1 and res.n_triangulated >= 150
    gt = tv.get()
    assert 0 < gt["triangulated"].sum() < 300
    a, b = DirectRefinement.bare(s.width, s.height, s.K4), DirectRefinement.bare(s.width, s.height, s.K4)
    for r in (a, b):
        r.set_frames(s.img1, s.img2, s.expo1, s.expo2)
    a.set_points_twoview(fl, tv)
    b.set_points_flow(fl, gt["triangulated"], gt["p3d"][:, 2])       # z = mvIniP3D[i].z / median_depth
    assert_same(a.points(), b.points())
    va, vb = a.videpth(), b.videpth()
    assert same(va, vb)
    tri = gt["triangulated"] != 0
    with np.errstate(all="ignore"):
        want = np.where(tri, (1.0 / gt["p3d"][:, 2].astype(np.float64)).astype(f32), f32(-1.0)).astype(f32)
    assert same(va, want)                                            # Initializer.cpp:155-159
    assert_same(refiner_outputs(a, s, refine=False), refiner_outputs(b, s, refine=False))
    for o_ in (a, b, tv, fl):
        o_.close()


def test_set_points_twoview_refusals_change_nothing():
    from hslam_amd._lib import HsError
    from hslam_amd.refine import DirectRefinement
    from test_gpu_init import fimgs, img8_of
    s, fl = tracked_flow()
    g = fl.get()
    sets = sets_for(g["good"])
    r = DirectRefinement.bare(s.width, s.height, s.K4)
    r.set_frames(s.img1, s.img2, s.expo1, s.expo2)
    r.set_points(s.u, s.v, s.tri, s.z)
    before = r.points()

    def refused(tv, flow):
        with pytest.raises(HsError, match=r"\(-5\)"):
            r.set_points_twoview(flow, tv)
        after = r.points()
        assert all(same(before[k], after[k]) for k in before)

    tv = TwoViewFit(300, s.K4)
    refused(tv, fl)                                                  # no fit yet
    assert tv.fit(g["first_xy"], g["xy"], g["good"], sets).ok == 1
    refused(tv, fl)                                                  # a host-fed fit belongs to no flow's first frame
    assert tv.fit_flow(fl, sets).ok == 1
    tv.check_rt(np.eye(3, dtype=f32)[None], np.array([[1, 0, 0]], f32), g["good"])
    refused(tv, fl)                                                  # a debug entry since
    assert tv.fit_flow(fl, sets).ok == 1
    s2, fl2 = tracked_flow(0.15)
    refused(tv, fl2)                                                 # another flow
    res = tv.fit_flow(fl2, sets_for(fl2.get()["good"]))
    assert res.ok == 0 and res.why in (3, 4)
    refused(tv, fl2)                                                 # the last fit did not succeed
    assert tv.fit_flow(fl, sets).ok == 1
    fl.set_first(img8_of(fimgs(s)[0]), g["first_xy"])
    refused(tv, fl)                                                  # the fit belongs to the first frame before
    for o_ in (r, tv, fl, fl2):
        o_.close()


# ---- 7. refusals: each leaves the last result readable

def test_refusals_leave_the_last_result_readable():
    from hslam_amd._lib import HsError
    s = tc.scene("general", 300)
    sets = tc.sets_of("general", 300, 200)
    tv, res = device_fit("general", 300, 200)
    want, want_g, want_rt = bytes(res), tv.get(), tv.get_rt()
    lib = tv.lib

    def unchanged():
        assert bytes(tv.last_result()) == want
        g, rt = tv.get(), tv.get_rt()
        assert all(same(g[k], want_g[k]) for k in g) and all(same(rt[k], want_rt[k]) for k in rt)

    bad = sets.copy()
    bad[7, 3] = 300                                                  # out of range
    with pytest.raises(HsError, match=r"\(-1\).*range"):
        tv.fit(s["xy1"], s["xy2"], s["status"], bad)
    unchanged()
    bad[7, 3] = -1
    with pytest.raises(HsError, match=r"\(-1\).*range"):
        tv.fit(s["xy1"], s["xy2"], s["status"], bad)
    unchanged()
    bad = sets.copy()
    bad[199, 7] = int(np.flatnonzero(s["status"] == 0)[0])           # a key with status 0
    with pytest.raises(HsError, match=r"\(-1\).*status"):
        tv.fit(s["xy1"], s["xy2"], s["status"], bad)
    unchanged()
    bad = sets.copy()
    bad[0, 5] = bad[0, 1]                                            # a repeated index
    with pytest.raises(HsError, match=r"\(-1\).*repeats"):
        tv.fit(s["xy1"], s["xy2"], s["status"], bad)
    unchanged()
    with pytest.raises(HsError, match=r"\(-1\).*n_sets"):
        tv.fit(s["xy1"], s["xy2"], s["status"], np.zeros((0, 8), np.int32))
    with pytest.raises(HsError, match=r"\(-1\).*n_sets"):
        tv.fit(s["xy1"], s["xy2"], s["status"], np.tile(sets, (2, 1))[:257])
    unchanged()
    big = tc.scene("general", 2049)
    with pytest.raises(HsError, match=r"\(-1\).*capacity"):          # n above the capacity
        tv.fit(big["xy1"], big["xy2"], big["status"], sets)
    unchanged()
    h = C.c_void_p()
    k = (C.c_double * 4)(*tc.K4)
    assert lib.hs_twoview_create(C.byref(h), 10 ** 6, 300, k) == -1 and not h.value      # another device
    assert lib.hs_twoview_create(C.byref(h), 0, 7, k) == -1 and not h.value
    unchanged()
    tv.close()


def test_status_rule_on_the_device_and_flow_refusals():
    """hs_twoview_fit_flow checks the status rule where the status is: on the device.  A refused fit changes nothing."""
    from hslam_amd._lib import HsError
    from hslam_amd.flow import KeypointFlow
    s, fl = tracked_flow()
    g = fl.get()
    sets = sets_for(g["good"], 20)
    tv = TwoViewFit(300, s.K4)
    fresh = KeypointFlow(s.width, s.height, 300)
    with pytest.raises(HsError, match=r"\(-5\)"):                    # before any fit
        tv.get()
    with pytest.raises(HsError, match=r"\(-5\).*track"):             # a flow that has not tracked
        tv.fit_flow(fresh, sets)
    res = tv.fit_flow(fl, sets)
    want, want_g = bytes(res), tv.get()
    bad = sets.copy()
    bad[11, 2] = int(np.flatnonzero(g["good"] == 0)[0])
    if bad[11, 2] in sets[11]:
        bad[11] = sets[10]
        bad[11, 2] = int(np.flatnonzero(g["good"] == 0)[0])
    with pytest.raises(HsError, match=r"\(-1\).*status"):
        tv.fit_flow(fl, bad)
    assert bytes(tv.last_result()) == want
    g2 = tv.get()
    assert all(same(g2[k], want_g[k]) for k in g2)
    small = TwoViewFit(100, s.K4)
    with pytest.raises(HsError, match=r"\(-1\).*capacity"):
        small.fit_flow(fl, sets)
    for o_ in (tv, small, fresh, fl):
        o_.close()


# ---- 8. lifetime

def test_create_use_destroy_returns_every_allocation():
    from hslam_amd._lib import load
    lib = load()
    lib.hs_debug_live_allocations.argtypes, lib.hs_debug_live_allocations.restype = [], C.c_longlong
    gc.collect()
    start = lib.hs_debug_live_allocations()
    s = tc.scene("general", 67)
    sets = np.ascontiguousarray(tc.sets_of("general", 67, 3))
    k = (C.c_double * 4)(*tc.K4)
    for _ in range(3):
        h = C.c_void_p()
        assert lib.hs_twoview_create(C.byref(h), 0, 67, k) == 0
        held = lib.hs_debug_live_allocations()
        assert held > start
        rc = lib.hs_twoview_fit(h, 67, s["xy1"].ctypes.data_as(C.c_void_p), s["xy2"].ctypes.data_as(C.c_void_p),
                                s["status"].ctypes.data_as(C.c_void_p), 3, sets.ctypes.data_as(C.c_void_p), None)
        assert rc == 0
        assert lib.hs_debug_live_allocations() == held              # nothing is allocated after create
        lib.hs_twoview_destroy(h)
        assert lib.hs_debug_live_allocations() == start
