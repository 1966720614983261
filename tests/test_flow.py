"""tests/flow_ref.py, the numpy statement of include/hs_flow.h's contract, checked on its own (no GPU): it recovers a
known sub-pixel shift, finds no flow between an image and itself, its pyramid and derivative give the hand-checkable
values, the level rule gives the stated level counts, and the coverage inputs that the GPU tests reuse reach every
exit reason at level 0.  Also builds and runs tests/c/flow_args_main.cpp, the argument checks of hs_flow.cpp, under
the host sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import flow_cases as cases
import flow_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "h-slam_amd", "lib")


@pytest.mark.parametrize("k", range(len(cases.SHIFT_CASES)))
def test_recovers_a_known_shift(k):
    a, b, pts, shift, r = cases.shift_case(k)
    flow = r["xy"] - pts
    d = np.abs(flow - shift).max(axis=1)
    print(f"{cases.SHIFT_CASES[k]}: |flow - shift| median {np.median(d):.4f} p90 {np.percentile(d, 90):.4f} "
          f"max {d.max():.4f}, err max {r['err'].max():.3f}, status {int(r['status'].sum())}/200")
    assert np.all(r["status"] == 1) and np.all(r["err"] < 7)
    assert d.max() < 0.1


@pytest.mark.parametrize("k", [0, 2])
def test_identity_has_no_flow(k):
    a, _, pts, _, _ = cases.shift_case(k)
    r = ref.calc(a, a, pts)
    assert np.all(r["status"] == 1)
    assert np.abs(r["xy"] - pts).max() < 1e-3
    assert np.all(r["err"] == 0)


def test_pyramid_and_derivative_by_hand():
    c = np.full((37, 52), 77, np.uint8)
    levels = ref.pyramid(c)
    assert [lv.shape for lv in levels] == [(37, 52), (19, 26)]    # (10, 13) would not be > 15
    assert all(np.all(lv == 77) for lv in levels)
    assert not ref.scharr(c).any()
    ramp = np.tile(np.arange(60, dtype=np.uint8), (40, 1))         # I = x
    d = ref.scharr(ramp)
    assert np.all(d[:, 1:-1, 0] == 32) and np.all(d[..., 1] == 0)
    assert np.all(d[:, [0, -1], 0] == 0)                            # reflect-101: both neighbours are the same pixel
    down = ref.pyr_down(ramp)
    assert down.shape == (20, 30)
    assert np.array_equal(down[:, 1:-1], np.tile(2 * np.arange(1, 29, dtype=np.uint8), (20, 1)))
    col = np.tile(np.arange(40, dtype=np.uint8)[:, None], (1, 60))  # I = y
    d = ref.scharr(col)
    assert np.all(d[1:-1, :, 1] == 32) and np.all(d[..., 0] == 0)
    rng = np.random.default_rng(0).integers(0, 256, size=(33, 47), dtype=np.uint8)
    d = ref.scharr(rng).astype(np.int32)
    assert np.abs(d).max() <= 4080


@pytest.mark.parametrize("size,levels", [((96, 80), 3), ((64, 48), 2), ((61, 61), 3), ((40, 40), 2), ((30, 30), 1)])
def test_level_rule(size, levels):
    assert ref.n_levels(*size) == levels
    assert len(ref.pyramid(np.zeros(size[::-1], np.uint8))) == levels


def test_coverage_inputs_reach_every_exit_reason_at_level_0():
    seen = set()
    for k in range(len(cases.COVERAGE_SIZES)):
        for with_init in (False, True):
            r = cases.coverage_case(k, with_init)[4]
            seen |= set(r["reasons"][:, 0].tolist())
            # a status-0 point has err 0 and the level-0 reasons that clear the status are the failing ones
            assert np.all(r["err"][r["status"] == 0] == 0)
            failing = np.isin(r["reasons"][:, 0], (ref.LEFT_IMAGE, ref.MIN_EIG, ref.PREV_OUTSIDE, ref.ERR_OUTSIDE))
            assert np.array_equal(failing, r["status"] == 0)
    no_init = set()
    for k in range(len(cases.COVERAGE_SIZES)):
        no_init |= set(cases.coverage_case(k)[4]["reasons"][:, 0].tolist())
    names = {ref.REASONS[c] for c in no_init}
    print("level-0 exit reasons without a guess:", sorted(names))
    assert no_init == set(range(7)), sorted(set(ref.REASONS) - names)
    assert seen == set(range(7))


def test_mean_flow_truncates_as_the_reference_does():
    prev = np.zeros((4, 2), np.float32)
    xy = np.array([[2.6, 0], [0, 2.6], [2.6, 0], [100, 100]], np.float32)
    good = np.array([1, 1, 1, 0], np.uint8)
    # (int)(0 + 2.6) = 2, (int)(2 + 2.6) = 4, (int)(4 + 2.6) = 6; a float sum would give 7.8 / 3
    assert ref.mean_flow(prev, xy, good) == np.float32(6) / np.float32(3)


def test_argument_checks_under_host_sanitizers(tmp_path):
    """hs_flow.cpp's argument validation returns before any device call: compiled with the host sanitizers together
    with tests/c/flow_args_main.cpp and run as a program of its own (nothing is loaded into Python)."""
    if not os.path.exists(os.path.join(LIBDIR, "libhslam_amd.so")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "h-slam_amd", "csrc")], check=True, capture_output=True)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "flow_args_main"
    # host side only: neither file defines a kernel, and the launch stubs come from the library
    subprocess.run([os.path.join(rocm, "bin", "hipcc"), "--cuda-host-only", "-std=c++17", "-O1", "-g", "-Wall",
                    "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-x", "hip",
                    os.path.join(ROOT, "tests", "c", "flow_args_main.cpp"),
                    os.path.join(ROOT, "h-slam_amd", "csrc", "hs_flow.cpp"), "-o", str(exe),
                    "-L", LIBDIR, "-lhslam_amd", "-Wl,-rpath," + LIBDIR], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 checks failed" in r.stdout
