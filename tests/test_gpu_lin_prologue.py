"""hs_k_lin's block prologue on windows that fill its tables only partly, at test_gpu_lin_onepoint's bars.

lin_block's prologue requests the block's constants, the stop word and the wave's first point in one batch: every
load is unconditional at a clamped index, the LDS stores are predicated, and the constants are spread over the
block's waves (precalc words on waves 4-7, xAd on wave 1, calib on wave 2, thresholds / calib step / image slots on
wave 3).  The 8-frame windows of the other tests fill every table to the brim (224 precalc words, 64 xAd entries,
8 thresholds), so a clamp or a store predicate that is off by a frame shows only on smaller windows:

* windows of 2, 3, 5 and 8 frames (make_ba_scene, seed 3) with 13 to 18 points per host: 56 to 224 precalc words,
  16 to 64 xAd entries, and in every host a block whose last waves hold no point (their clamped point loads
  are issued all the same);
* the 3-frame window without host 0.

Each is linearized (hs_ba_linearize) and compared with the oracle, then run through hs_ba_iterate(0, 2), whose
second launch applies the fused point step with the block's K.xad / K.cs / K.th; the step is compared bit for bit
with the granular path on a twin window (hs_ba_solve_system's resubstitute kernel takes xAd from the solve, not
from the prologue).  The 3-frame window also runs the linearizeAll(true) and the marginalization instantiations
against the oracle, in both accumulation orders, and the device-side break: the launches after the break return
at the prologue's stop word, before any store.
"""
import copy

import numpy as np
import pytest

from test_gpu_ba import _close_b, _close_H, _pair
from test_gpu_fp64_model import ba_window
from test_gpu_lin_onepoint import WAVES, _arms, _assert_residuals, _assert_systems, _partition, _subset

pytestmark = pytest.mark.gpu

POINTS = {2: 26, 3: 45, 5: 90, 8: 104}  # 13, 15, 18 and 13 points per host: blocks of 6 to 8 points


@pytest.fixture(scope="module")
def windows():
    from hslam_amd.scene import make_ba_scene
    cache = {}

    def get(nF):
        if nF not in cache:
            cache[nF] = make_ba_scene(n_points=POINTS[nF], n_frames=nF, seed=3)
        return cache[nF]
    return get


def _window(windows, name):
    if name == "3_no_host0":
        s = windows(3)
        s = _subset(s, s.pt_host != 0)
        assert _partition(s)[0] == []
    else:
        s = windows(int(name))
    part = _partition(s)
    per_host = [sum(p) for p in part if p]
    assert all(12 <= n <= 20 for n in per_host), per_host
    # every populated host has a block with waves that hold no point; no wave holds two
    assert all(any(_arms(b)[2] > 0 for b in p) for p in part if p)
    assert all(_arms(b)[1] == 0 for p in part for b in p)
    return s, part


@pytest.mark.parametrize("name", ["2", "3", "5", "8", "3_no_host0"])
def test_partly_filled_tables(name, windows):
    from oracle_ffi import OracleBA
    s, part = _window(windows, name)
    g, twin = ba_window(s, False), ba_window(s, False)
    p = g.partition()
    assert p["kernel"] == "hs_k_lin" and p["waves"] == WAVES and p["blocks"] == sum(len(x) for x in part), p

    # ---- hs_ba_linearize (the fused point step off) against the oracle
    eg = g.linearizeAll(reset=True)
    twin.linearizeAll(reset=True)
    o = OracleBA(s)
    eo = o.linearize_all(reset=True)
    o.apply_res()
    _assert_residuals(g.residuals(), o.residuals(), np.ones(s.n_res, bool), "linearize")
    assert abs(eg - eo) <= 1e-9 * abs(eo)
    assert np.array_equal(g.frames()["energyTH"], o.frames()["energyTH"])
    _assert_systems(g, o, "linearize")
    pg, po = g.points(), o.points()
    for k in ("HdiF", "bdSumF"):
        assert np.array_equal(pg[k], po[k]), k

    # ---- the fused point step (the second launch of iterate(0, 2)) against the granular path on the twin
    e2 = g.iterate(0, 2)
    e1 = twin.iterate(0, 1)
    assert e2[0] == e1[0]
    p1 = twin.points()
    xt = twin.solveSystem(1)
    step_t = twin.points()["step"].copy()
    twin.doStepFromBackup()
    f2, p2 = g.frames(), g.points()
    moved = p2["step"] != 0
    print(f"{name}: {s.n_points} points, {s.n_res} residuals, {int(moved.sum())} points stepped, "
          f"|x| max {np.abs(xt).max():.3e}, calib step {xt[:4]}")
    assert np.abs(xt).max() > 0 and moved.any()
    assert np.array_equal(p2["step"], step_t)
    assert np.array_equal(p2["idepth"], twin.points()["idepth"])
    assert np.array_equal(p2["idepth"], (p1["idepth"] + p2["step"]).astype(np.float32))
    assert np.array_equal(f2["state"], twin.frames()["state"])
    g.close()
    twin.close()


@pytest.mark.parametrize("exact", [True, False])
def test_fix_instantiation_three_frames(exact, windows):
    """linearizeAll(true) (hs_k_lin_exact_fix / hs_k_lin_fix) on the 3-frame window: test_gpu_ba's
    test_fix_linearization_bit_exact, whose per-residual and per-point outputs do not depend on the order."""
    scene = windows(3)
    g, o = _pair(scene, exact=exact)
    g.linearizeAll(reset=True)
    o.linearize_all(reset=True)
    o.apply_res()
    rng = np.random.default_rng(5)
    rb0 = rng.uniform(0.0, 0.02, scene.n_points).astype(np.float32)
    ng0 = rng.integers(0, 5, scene.n_points).astype(np.int32)
    out = g.fixLinearization(rb0, ng0)
    eo, drop_o, rb_o, ng_o = o.fix_linearization(rb0, ng0)
    rg, ro = g.residuals(), o.residuals()
    assert np.array_equal(rg["state"], ro["state"])
    assert np.array_equal(out["drop"], drop_o)
    act = ro["state"] == 0
    assert act.any()
    assert np.array_equal(rg["energy"], ro["energy"].astype(np.float32))
    assert np.array_equal(rg["center"][act], ro["center"][act])
    assert np.array_equal(out["maxRelBaseline"], rb_o)
    assert np.array_equal(out["numGoodResiduals"], ng_o)
    assert abs(out["energy"] - eo) <= 1e-9 * abs(eo)
    fg, fo = g.frames(), o.frames()
    assert np.array_equal(fg["state"], fo["state"])
    assert np.array_equal(fg["pose"], fo["pose"])
    assert np.array_equal(fg["energyTH"], fo["energyTH"])
    g.close()


@pytest.mark.parametrize("exact", [True, False])
def test_marg_instantiation_three_frames(exact, windows):
    """The marginalization pass (hs_k_lin_exact_marg / hs_k_lin_marg) on the 3-frame window:
    test_gpu_ba's test_marginalize_points (the frames carry a state offset, so adHTdeltaF is live)."""
    s = copy.copy(windows(3))
    rng = np.random.default_rng(11)
    st = np.zeros((s.n_frames, 10))
    st[1:, :6] = rng.normal(size=(s.n_frames - 1, 6)) * 2e-3
    st[1:, 6:8] = rng.normal(size=(s.n_frames - 1, 2)) * 1e-3
    s.frames_state = st
    g, o = _pair(s, exact=exact)
    g.linearizeAll(reset=True)
    o.linearize_all(reset=True)
    o.apply_res()
    pts = np.nonzero(s.pt_host == 0)[0][::2]
    HMg, bMg = g.marginalizePointsF(pts)
    HMo, bMo = o.marginalize_points(pts)
    assert np.abs(HMo).max() > 0 and np.abs(bMo).max() > 0
    okH, rH = _close_H(HMg, HMo)
    okb, rb = _close_b(bMg, bMo, HMo)
    assert okH, f"HM worst ratio {rH}"
    assert okb, f"bM worst ratio {rb}"
    rg, ro = g.residuals(), o.residuals()
    assert np.array_equal(rg["state"], ro["state"])
    assert np.array_equal(rg["energy"], ro["energy"].astype(np.float32))
    g.close()


def test_break_three_frames(windows, monkeypatch):
    """optimize(allow_break=True) on the 3-frame window with the break decided on the device and on the host
    (HS_HOST_BREAK=1), as test_gpu_ba's test_optimize_break_device_matches_host does at 2k.  thOptIterations is
    huge, so every step allows the break and the run stops after iteration minOptIterations: the device run has
    launched the remaining iterations already, and each of those launches returns at the stop word.  The host run
    launches nothing after the break, so every buffer the C ABI reads back must be equal between the two."""
    from hslam_amd._lib import default_params
    from hslam_amd.ba import BAWindow
    scene = windows(3)
    runs = []
    for host in ("0", "1"):
        monkeypatch.setenv("HS_HOST_BREAK", host)
        params = default_params()
        params.thOptIterations = 1e9
        params.minOptIterations = 1
        g = BAWindow(scene, params=params)
        n, e = g.optimize(6, allow_break=True)
        runs.append((n, e, g.frames(), g.points(), g.residuals()))
        g.close()
    (n0, e0, f0, p0, r0), (n1, e1, f1, p1, r1) = runs
    assert n0 == n1 == 2, (n0, n1)  # iterations 0 and 1 ran; the call asked for more
    assert np.array_equal(e0, e1)
    for a, b in ((f0, f1), (p0, p1), (r0, r1)):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), k
