"""hs_k_solve's panel LDLT after its main loop's instruction count was cut (the carry published unmasked, a
diagonal row's pivot stored from the row's own registers): the checks that would show a wrong mask, a stale word of
L^T, of the pivots or of the diagonal rows' rhs, on the windows, cases and bars of tests/test_gpu_solve_model.py
(device_run and bar are imported from there; the runs are shared with that file through device_run's cache).

Window sizes.  2, 7 and 8 frames (n = 20, 60, 68) are, in order, the shortest main loop (four phases), the largest
system whose rows fit the panel wave's 64 lanes with clamped lanes beyond n, and the only size that runs the rows
64-67 path.  The window API takes 2 ... 8 frames (hs_ba_set_window refuses one frame), so the residual check covers
n = 20, 28, ..., 68 and n = 12 is left to the harness tools/micro/ldlt_chain.hip.

Cases.  Without a marginalization prior: photo_it0; with one: fej_it1.  Both are solves without the gauge projection
(iteration < 2), so HFinal x = b holds for the x that is read back.

Residual bar.  With A = S HFinal S (lower triangle mirrored, the matrix the LDLT factors), y = x / S and c = S b, a
backward-stable factorization leaves |A y - c| <= g n eps |A| |y| <= g n eps cond(A) |c|; g = 64 is the margin
test_gpu_solve_model gives a blocked LDLT without pivoting, so the bar is 64 n 2^-52 cond(A) max|c| on max|A y - c|,
with the model's scaling and cond (test_solve_model.system_figures).  An L entry stored over a zero of L^T, or one
that was masked away, changes A y - c in that row at the size of the entry, which the x bar of a small block can hide.

Dead pivots.  The solve scales by 1 / sqrt(diag(HFinal) + 10) and the frame and calibration priors keep that diagonal
positive, so no window reaches a pivot with |d| <= DBL_MIN through the public API; the reciprocal's guard is covered
by the harness (a system with an exact zero pivot in the last panel), not here.
"""
import numpy as np
import pytest

import solve_model as sm
from test_gpu_solve_model import bar, device_inputs, device_run, device_window
from test_solve_model import CEIL, NFS, metrics, model_x, system_figures

pytestmark = pytest.mark.gpu

EDGE = [(nF, v) for nF in (2, 7, 8) for v in ("photo_it0", "fej_it1")]       # without / with a prior
ALL = [(nF, v) for nF in NFS for v in ("photo_it0", "fej_it1")]
SYS = ("HA", "bA", "HL", "bL", "Hsc", "bsc", "HM", "bM", "delta")


def ident(c):
    return f"{c[0]}f-{c[1]}"


@pytest.mark.parametrize("case", EDGE, ids=ident)
def test_edge_windows_against_model(case):
    r = device_run(*case)
    o = r["oracle"]
    So, _, _ = system_figures(o["inp"])
    do_x, do_blk, _ = metrics(o["x"], model_x(o["inp"], o["iteration"]), So)
    S, cond, floor = system_figures(r["inp"])
    assert len(S) == 4 + 8 * case[0]
    dg_x, dg_blk, which = metrics(r["x"], model_x(r["inp"], r["iteration"]), S)
    bx, bb = bar(do_x, floor), bar(do_blk, floor)
    print(f"{ident(case)}: n {len(S)}  cond {cond:.2e}  d_oracle x {do_x:.2e} blocks {do_blk:.2e}  d_device x {dg_x:.2e} "
          f"blocks {dg_blk:.2e} ({which})  bar x {bx:.2e} blocks {bb:.2e}")
    assert do_x <= CEIL and do_blk <= CEIL, (do_x, do_blk)
    assert np.all(np.isfinite(r["x"]))
    assert dg_x <= bx and dg_blk <= bb, (dg_x, bx, dg_blk, bb, which)


@pytest.mark.parametrize("case", EDGE, ids=ident)
def test_second_solve_of_the_same_system_is_bit_equal(case):
    """A second context of the same window (solveSystem consumes the system) holds bit-identical systems, and its x
    equals the first one's bit for bit: the launch starts from whatever the previous launches left in LDS, so a lane
    reading a word of L^T, the pivots or the diagonal rhs that this launch did not write would show here."""
    r = device_run(*case)
    g, _, _, calib_zero, _, _ = device_window(*case)
    inp = device_inputs(g, calib_zero)
    for k in SYS:
        assert np.array_equal(inp[k], r["inp"][k]), k
    x = g.solveSystem(r["iteration"])
    g.close()
    assert np.array_equal(x, r["x"])


@pytest.mark.parametrize("case", ALL, ids=ident)
def test_system_times_x_reproduces_b(case):
    r = device_run(*case)
    inp = r["inp"]
    assert r["iteration"] < 2                                    # no gauge projection: x solves the system itself
    H, b = sm.final_system(*[inp[k] for k in SYS])
    S, cond, floor = system_figures(inp)
    A = sm.lower_mirrored(S[:, None] * H * S[None, :])
    y, c = r["x"] / S, S * b
    res = np.abs(A @ y - c)
    worst = int(res.argmax())
    br = 64 * floor * np.abs(c).max()
    print(f"{ident(case)}: n {len(S)}  cond {cond:.2e}  max |A y - c| {res.max():.2e} (row {worst})  max |c| "
          f"{np.abs(c).max():.2e}  bar {br:.2e}")
    assert res.max() <= br, (res.max(), br, worst)
