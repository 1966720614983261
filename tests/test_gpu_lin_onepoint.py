"""hs_k_lin's arms that the headline window never mixes, against the oracle at test_gpu_photo's bars.

A wave of hs_k_lin that holds one point runs it outside the point loop (lin_block's one-point arm); a wave with more
runs the loop.  The 8 x 2000 headline has one point per wave everywhere, its blocks are full and every point has
seven listed residuals.  The windows here have

* blocks whose last waves carry no point (2 x 16 and 3 x 64 points);
* a host of 17 points in a window large enough for two points per wave: its first block holds 8 points (every wave
  in the one-point arm), its second 9 (wave 0 loops over two) -- the partition is computed from the host and block
  boundaries and asserted;
* the same window without host 0 (no point ahead of the first block's host);
* in every window a point with an empty residual list and a point whose every projection leaves the image.

Each window is linearized (hs_ba_linearize: the fused point step off) and compared with the oracle, then run through
one hs_ba_iterate(0, 2) (two solves, each followed by the production launch with the fused step) and compared with
the oracle placed at the device's state: the frames' states and the depths after the second step, the frame
thresholds that launch read (those a twin window holds after one iteration).  The oracle linearizes from reset
there, so it gets the window without the residuals the device holds out of the image (that state is sticky and keeps
the residual's last energy, which the twin gives).  The C ABI reads back neither the active masks nor Hcd: they are covered by
what they feed, the residuals' active flags, the Schur-complement system (which = 2) and the next point step.

The fused point step itself (resubstitute + the point part of doStepFromBackup inside the launch) is compared bit
for bit with the granular path on the twin (hs_ba_solve_system's resubstitute kernel + hs_ba_do_step), which walks
the point's residual list with a plain loop; the oracle cannot serve there, its x differs from the device's at the
1e-3 level (test_gpu_ba.test_solve_and_step).

The C ABI has no read-back of the block boundaries either: _partition restates make_partition (hs_ba.cpp) and
lin_block's shares, WAVES / BLOCKS_TARGET restate HS_LIN_NW / kLinBlocksTarget, and the device is asked for its block
count and wave count only.  A change of the partition rule that keeps the count has to be carried over to here.
"""
import copy

import numpy as np
import pytest

import photo_cases as pc
from test_gpu_ba import _close_b, _close_H
from test_gpu_fp64_model import ba_window

pytestmark = pytest.mark.gpu

WAVES = 8            # HS_LIN_NW
BLOCKS_TARGET = 256  # kLinBlocksTarget
OOB = 1              # HS_RES_OOB
FAR = np.float32(50.0)  # an inverse depth that moves every projection by more than the image's width


def _subset(scene, keep):
    """The window with the points keep[p] only (and their residuals)."""
    keep = np.asarray(keep, bool)
    remap = -np.ones(scene.n_points, np.int64)
    remap[keep] = np.arange(keep.sum())
    rsel = keep[scene.res_point]
    s = copy.copy(scene)
    for name in ("pt_host", "pt_u", "pt_v", "pt_idepth", "pt_idepth_zero", "pt_color", "pt_weights", "pt_idepth_true"):
        setattr(s, name, np.ascontiguousarray(getattr(scene, name)[keep]))
    s.res_point = remap[scene.res_point[rsel]].astype(np.int32)
    s.res_target = np.ascontiguousarray(scene.res_target[rsel])
    return s


def _edge_points(scene):
    """The window with one point's residual list emptied and another point moved out of every target's image; both
    are taken from the middle of the first populated host.  Returns (scene, empty point, far point)."""
    h0 = scene.pt_host[0]
    n0 = int((scene.pt_host == h0).sum())
    p_empty, p_far = n0 // 2, n0 // 2 + 1
    assert scene.pt_host[p_far] == h0
    s = copy.copy(scene)
    rsel = scene.res_point != p_empty
    s.res_point = np.ascontiguousarray(scene.res_point[rsel])
    s.res_target = np.ascontiguousarray(scene.res_target[rsel])
    s.pt_idepth = scene.pt_idepth.copy()
    s.pt_idepth[p_far] = FAR
    s.pt_idepth_zero = s.pt_idepth.copy()
    assert (s.res_point == p_far).sum() > 0
    return s, p_empty, p_far


def _partition(scene):
    """hs_k_lin's blocks (make_partition, lin_block): per host the list of its blocks' point counts."""
    nP, nF = scene.n_points, scene.n_frames
    ppw = max(1, -(-nP // (WAVES * BLOCKS_TARGET)))
    out = []
    for h in range(nF):
        nh = int((scene.pt_host == h).sum())
        nb = -(-nh // (WAVES * ppw)) if nh else 0
        out.append([nh * (q + 1) // nb - nh * q // nb for q in range(nb)])
    return out


def _arms(sizes):
    """(waves in the one-point arm, waves in the loop arm, waves without a point) of a block of `sizes` points."""
    per_wave = [len(range(w, sizes, WAVES)) for w in range(WAVES)]
    return sum(n == 1 for n in per_wave), sum(n > 1 for n in per_wave), sum(n == 0 for n in per_wave)


@pytest.fixture(scope="module")
def big_window():
    """8 frames x 300 points at 160 x 120: the base of the two-points-per-wave windows."""
    return pc.make_photo_ba(8, 2400, "photo")


def _case(name, big):
    if name == "2x16":
        # seed 1: the two-frame window whose residuals stay IN through the GN steps (the default seed's first step
        # throws every residual OUT, so its second fused step would move no point)
        s = pc.make_photo_ba(2, 16, "photo", seed=1)
        want = [[8], [8]]
    elif name == "3x64":
        s = pc.make_photo_ba(3, 64, "photo")
        want = None
    else:
        keep = np.ones(big.n_points, bool)
        h0 = np.nonzero(big.pt_host == 0)[0]
        keep[h0[17 if name == "mixed" else 0:]] = False
        s = _subset(big, keep)
        want = None
    s, p_empty, p_far = _edge_points(s)
    part = _partition(s)
    if name == "2x16":
        assert part == want
    elif name == "3x64":
        # 22 + 21 + 21 points: three blocks a host, the last with waves that carry no point
        assert [sum(p) for p in part] == [22, 21, 21] and all(len(p) == 3 for p in part)
        assert any(_arms(b)[2] > 0 for p in part for b in p)
        assert all(_arms(b)[1] == 0 for p in part for b in p)
    elif name == "mixed":
        # host 0: 17 points at two points per wave -> blocks of 8 and 9: the first all one-point waves, the second
        # with wave 0 in the loop arm and the others in the one-point arm
        assert s.n_points > WAVES * BLOCKS_TARGET and part[0] == [8, 9]
        assert _arms(8) == (8, 0, 0) and _arms(9) == (7, 1, 0)
    else:
        assert s.n_points > WAVES * BLOCKS_TARGET and part[0] == [] and len(part[1]) > 0
    return s, p_empty, p_far, part


def _assert_residuals(rg, ro, sel, what):
    """test_gpu_photo's per-residual asserts on the residuals sel."""
    assert np.array_equal(rg["state"][sel], ro["state"][sel]), what
    active_o = (ro["state"] == 0) & sel
    assert active_o.any(), what
    assert np.array_equal(rg["active"].astype(bool)[sel], (ro["state"] == 0)[sel]), what
    assert np.array_equal(rg["energy"][sel], ro["energy"].astype(np.float32)[sel]), what
    assert np.array_equal(rg["energy_wo"][sel], ro["energy_wo"].astype(np.float32)[sel]), what
    assert np.array_equal(rg["JpJdF"][active_o], ro["JpJdF"][active_o]), what
    assert np.array_equal(rg["center"][active_o], ro["center"][active_o]), what


def _assert_systems(g, o, what):
    for which in (0, 2):
        Ho, bo = o.accumulate(which)
        Hg, bg = g.system(which)
        okH, rH = _close_H(Hg, Ho)
        okb, rb = _close_b(bg, bo, Ho)
        assert okH, f"{what} which={which} H worst ratio {rH}"
        assert okb, f"{what} which={which} b worst ratio {rb}"


@pytest.mark.parametrize("name", ["2x16", "3x64", "mixed", "no_host0"])
def test_lin_arms_against_oracle(name, big_window):
    from oracle_ffi import OracleBA
    s, p_empty, p_far, part = _case(name, big_window)
    g, twin = ba_window(s, False), ba_window(s, False)
    p = g.partition()
    assert p["kernel"] == "hs_k_lin" and p["waves"] == WAVES and p["blocks"] == sum(len(x) for x in part), p
    far_res = s.res_point == p_far
    every = np.ones(s.n_res, bool)

    # ---- the fused step off: hs_ba_linearize from reset
    eg = g.linearizeAll(reset=True)
    twin.linearizeAll(reset=True)
    o = OracleBA(s)
    eo = o.linearize_all(reset=True)
    o.apply_res()
    r0, ro = g.residuals(), o.residuals()
    _assert_residuals(r0, ro, every, "linearize")
    assert np.all(r0["state"][far_res] == OOB)
    assert abs(eg - eo) <= 1e-9 * abs(eo)
    assert np.array_equal(g.frames()["energyTH"], o.frames()["energyTH"])
    _assert_systems(g, o, "linearize")
    pg, po = g.points(), o.points()  # the oracle's Schur prelude is formed by its accumulate(2)
    for k in ("HdiF", "bdSumF"):
        assert np.array_equal(pg[k], po[k]), k
    assert pg["HdiF"][p_empty] == 0 and pg["HdiF"][p_far] == 0 and pg["bdSumF"][p_empty] == 0

    # ---- the fused step on: two GN iterations on the device; the twin stops after the first
    e2 = g.iterate(0, 2)
    e1 = twin.iterate(0, 1)
    assert e2[0] == e1[0]
    r1, t1, p1 = twin.residuals(), twin.frames(), twin.points()
    f2, p2, r2 = g.frames(), g.points(), g.residuals()
    # the fused step against the granular path: the twin, bit for bit where g stood before its second iteration,
    # solves the same system with hs_ba_solve_system, whose resubstitute kernel (hs_k_resub: point_step, a plain
    # loop over the point's list that breaks at its end and skips the slots outside the active mask) forms the point
    # steps from the same per-point data, and applies them with hs_ba_do_step.  x, every point's step, the depths and
    # the frame states must be the fused launch's bit for bit.
    xt = twin.solveSystem(1)
    step_t = twin.points()["step"].copy()
    twin.doStepFromBackup()
    assert np.abs(xt).max() > 0
    assert np.array_equal(p2["step"], step_t)
    assert np.array_equal(p2["idepth"], twin.points()["idepth"])
    assert np.array_equal(f2["state"], twin.frames()["state"])
    # what the compared steps cover: every list is shorter than 8 (at most nF - 1 entries); points that moved, and
    # among them points with a listed residual outside the active mask (skipped in the middle of the list)
    n_listed = np.bincount(s.res_point, minlength=s.n_points)
    n_active = np.bincount(s.res_point, weights=r1["active"].astype(bool), minlength=s.n_points).astype(int)
    moved = p2["step"] != 0
    assert n_listed.max() < 8 and moved.any() and np.all(n_active[moved] > 0)
    skipping = moved & (n_active < n_listed)
    print(f"{name}: {int(moved.sum())} points stepped, {int(skipping.sum())} of them with a listed inactive residual, "
          f"list lengths {sorted(set(n_listed[moved].tolist()))}")
    assert skipping.any() or s.n_frames == 2  # (two frames: one entry per list)
    assert np.array_equal(p2["idepth"], (p1["idepth"] + p2["step"]).astype(np.float32))
    assert p2["step"][p_empty] == 0 and p2["step"][p_far] == 0 and p2["idepth"][p_far] == FAR
    # the residuals out of the image: found there before this launch (sticky: r0, r1) or by it.  Each keeps the
    # energy it had (applyRes) and counts with it in the launch's energy; the oracle gets the window without them
    sticky = (r0["state"] == OOB) | (r1["state"] == OOB)
    gone = r2["state"] == OOB
    assert np.all(gone[sticky]) and np.all(gone[far_res])
    assert not r2["active"][gone].any() and np.all(r2["energy_wo"][gone] == -1)
    assert np.array_equal(r2["energy"][gone], r1["energy"][gone])
    s2 = copy.copy(s)
    s2.frames_state = f2["state"].copy()
    s2.frames_energyTH = t1["energyTH"].copy()
    s2.pt_idepth = p2["idepth"].copy()
    s2.pt_idepth_zero = s2.pt_idepth.copy()
    s2.res_point = np.ascontiguousarray(s.res_point[~gone])
    s2.res_target = np.ascontiguousarray(s.res_target[~gone])
    o2 = OracleBA(s2)
    o2.set_calib(f2["calib"].copy())
    eo2 = o2.linearize_all(reset=True)
    o2.apply_res()
    ro2 = o2.residuals()
    print(f"{name}: {s.n_points} points, {s.n_res} residuals, out of the image {int(sticky.sum())} before the launch, "
          f"{int(gone.sum())} after it; {int((ro2['state'] == 0).sum())} active")
    _assert_residuals({k: v[~gone] for k, v in r2.items()}, ro2, np.ones(s2.n_res, bool), "iterate")
    e_gone = float(np.sum(r1["energy"][gone].astype(np.float64)))
    assert abs(e2[1] - (eo2 + e_gone)) <= 1e-9 * abs(eo2 + e_gone)
    assert np.array_equal(f2["energyTH"], o2.frames()["energyTH"])
    _assert_systems(g, o2, "iterate")
    po2 = o2.points()
    for k in ("HdiF", "bdSumF"):
        assert np.array_equal(p2[k], po2[k]), k
    assert p2["HdiF"][p_empty] == 0 and p2["HdiF"][p_far] == 0
    g.close()
    twin.close()
