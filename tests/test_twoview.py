"""The two-view fit without a GPU: the numpy model of include/hs_twoview.h (tests/twoview_ref.py) against properties
it must have, the host run of the very Jacobi and decision inlines the kernels call (tests/c/twoview_main.cpp on
h-slam_amd/csrc/hs_jacobi.h and hs_twoview_rule.h, built with -fsanitize=address,undefined), and the spread of the model
itself, which sets the bar of the GPU test of the hypothesis matrices."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-slam_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import twoview_cases as tc  # noqa: E402
import twoview_ref as tr  # noqa: E402
from hslam_amd.twoview import TwoViewResult, draw_sets  # noqa: E402  (fails before the feature exists)

f32 = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("twoview") / "twoview_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    os.path.join(ROOT, "tests", "c", "twoview_main.cpp"), "-o", str(out)], check=True)
    return str(out)


def run(exe, mode, text):
    out = subprocess.run([exe, mode], input=text, capture_output=True, text=True, check=True)
    assert out.stderr == "", out.stderr          # the sanitizers report there
    return [ln.split() for ln in out.stdout.split("\n") if ln]


def bits(f):
    return int(np.array([f], f32).view(np.uint32)[0])


# ---- 1. the model against rules: properties of the model, not parity bars

@pytest.mark.parametrize("kind, model", [("general", 1), ("planar", 0)])
def test_noise_free_scene_recovers_the_generating_motion(kind, model):
    s = tc.scene(kind, 300, 0, True)
    o = tr.fit(s["xy1"], s["xy2"], s["status"], tc.sets_of(kind, 300, 200, 0, True), tc.K4)
    assert o["ok"] == 1 and o["why"] == 0 and o["model"] == model
    assert o["n_triangulated"] == 300 and np.all(o["triangulated"] == 1)
    ang, dirn = tc.rotation_angle(o["R"], s["R"]), tc.direction_error(o["t"], s["t"])
    print(f"{kind}: rotation error {ang:.3e} rad, 1 - cos of the t direction {dirn:.3e}")
    assert ang < 1e-4 and dirn < 1e-4
    # the scaling of Initialize (:142-148): the median of the scaled depths is 1, t is scaled by the same number
    z = o["p3d"][o["triangulated"] == 1, 2]
    assert np.sort(z)[(len(z) - 1) // 2] == f32(1.0)
    assert abs(np.linalg.norm(o["t"]) * o["median_depth"] - 1) < 1e-5


@pytest.mark.parametrize("kind, whys", [("rotation", (3, 4)), ("outlier", (3, 4)), ("degenerate", (1, 2, 3, 4))])
def test_scenes_the_reference_refuses(kind, whys):
    s = tc.scene(kind, 300)
    o = tr.fit(s["xy1"], s["xy2"], s["status"], tc.sets_of(kind, 300, 200), tc.K4)
    assert o["ok"] == 0 and o["why"] in whys
    assert not o["triangulated"].any() and not o["R"].any() and not o["t"].any()


def test_noisy_routes():
    g = tc.scene("general", 300)
    o = tr.fit(g["xy1"], g["xy2"], g["status"], tc.sets_of("general", 300, 200), tc.K4)
    assert o["model"] == 1 and o["ok"] == 1
    assert tc.rotation_angle(o["R"], g["R"]) < 0.05 and tc.direction_error(o["t"], g["t"]) < 0.05
    # no outlier and no key with status 0 is triangulated
    assert not (o["triangulated"][(g["status"] == 0)]).any()
    p = tc.scene("planar", 300)
    o = tr.fit(p["xy1"], p["xy2"], p["status"], tc.sets_of("planar", 300, 200), tc.K4)
    assert o["model"] == 0


def test_sum256_is_the_documented_order():
    rng = np.random.default_rng(5)
    x = rng.normal(size=1000) * 10.0 ** rng.integers(-8, 8, 1000)
    part = [0.0] * 256
    for i, v in enumerate(x):
        part[i % 256] = part[i % 256] + float(v)
    s = 128
    while s:
        for t in range(s):
            part[t] = part[t] + part[t + s]
        s >>= 1
    assert tr.sum256(x) == part[0]
    assert abs(tr.sum256(x) - np.sum(x)) <= 1e-9 * np.abs(x).sum()


def test_draw_sets_is_the_reference_draw():
    status = np.ones(30, np.uint8)
    status[[3, 17]] = 0
    sets = draw_sets(50, status, np.random.default_rng(1))
    assert sets.shape == (50, 8) and sets.dtype == np.int32
    assert all(len(set(r)) == 8 for r in sets.tolist()) and status[sets].all()
    # uniform(0, size - 1) excludes its upper bound: the first draw never takes the last available key
    assert 29 not in sets[:, 0]
    only = draw_sets(3, np.ones(8, np.uint8), np.random.default_rng(2))
    assert all(sorted(r) == list(range(8)) for r in only.tolist())


def test_result_record_is_128_bytes():
    import ctypes
    assert ctypes.sizeof(TwoViewResult) == 128


# ---- 2. the inlines on the host

CASES = [("general", 67, 200), ("general", 300, 200), ("general", 2049, 200), ("planar", 67, 200), ("planar", 300, 200),
         ("planar", 2049, 200), ("degenerate", 300, 200), ("general", 8, 1), ("general", 40, 3)]


def design(kind, n, ns):
    s = tc.scene(kind, n)
    return tr.design_matrices(s["xy1"], s["xy2"], tc.sets_of(kind, n, ns))[:2]


def canon(M, like=None):
    """Unit Frobenius norm, the sign that makes the entry largest in `like` positive."""
    M = np.asarray(M, np.float64).reshape(len(M), -1)
    like = M if like is None else np.asarray(like, np.float64).reshape(len(M), -1)
    j = np.argmax(np.abs(like), axis=1)
    sg = np.sign(M[np.arange(len(M)), j])
    return M * (sg / np.linalg.norm(M, axis=1))[:, None]


def test_jacobi_null_vectors_against_numpy_svd(exe):
    worst = 0.0
    for kind, n, ns in CASES:
        for A in design(kind, n, ns):
            A = A[:40]                                     # 40 sets of every case through the program
            text = "".join(f"{a.shape[0]} " + " ".join(float(x).hex() for x in a.ravel()) + "\n" for a in A)
            rows = run(exe, "null", text)
            got = np.array([[float.fromhex(x) for x in r[:9]] for r in rows])
            sweeps = np.array([int(r[9]) for r in rows])
            assert got.shape == (len(A), 9) and sweeps.max() <= 16
            # the numpy restatement of the same code is the same arithmetic: equal to the last bit
            assert np.array_equal(got, tr.null_vector(A)), (kind, n)
            _, sv, vt = np.linalg.svd(A)
            ref = vt[:, 8] if A.shape[1] == 16 else np.array([np.linalg.svd(a)[2][8] for a in A])
            gap = sv[:, 7] / sv[:, 0]
            ok = gap > 1e-6                                # below it the null vector is not defined
            err = np.abs(canon(got) - canon(ref, got)).max(axis=1)
            # both factorizations are backward stable: each null vector is exact for A + dA, |dA| <= c eps sigma_1 with
            # a modest c, so each is within c eps sigma_1 / sigma_8 of the true one; c = 32 for a 16 x 9 matrix
            bar = 2 * 32 * 2.0 ** -53 / gap
            assert np.all(err[ok] <= bar[ok]), (kind, n, float((err[ok] / bar[ok]).max()))
            worst = max(worst, float((err[ok] / bar[ok]).max()))
            assert np.all(np.abs(np.linalg.norm(got, axis=1) - 1) < 1e-14)
    print(f"largest null-vector error / bar: {worst:.3f}")


def test_jacobi_4x4_and_svd3_match_the_numpy_restatement(exe):
    rng = np.random.default_rng(3)
    A4 = rng.normal(size=(50, 4, 4))
    A4[:10, 3] = A4[:10, 0] + A4[:10, 1]                   # exactly singular
    rows = run(exe, "null4", "".join(" ".join(float(x).hex() for x in a.ravel()) + "\n" for a in A4))
    got = np.array([[float.fromhex(x) for x in r] for r in rows])
    assert np.array_equal(got, tr.null_vector(A4))
    assert np.abs(np.einsum("bij,bj->bi", A4[:10], got[:10])).max() < 1e-13
    for rank3 in (0, 1):
        for k in range(20):
            A = rng.normal(size=(3, 3))
            if not rank3:
                A[:, 2] = 0.3 * A[:, 0] - 0.8 * A[:, 1]    # rank 2, like an essential matrix
            r = run(exe, "svd3", f"{rank3} " + " ".join(float(x).hex() for x in A.ravel()) + "\n")[0]
            v = np.array([float.fromhex(x) for x in r])
            U, w, Vt = tr.svd3(A, bool(rank3))
            assert np.array_equal(v[:9].reshape(3, 3), U) and np.array_equal(v[9:12], w)
            assert np.array_equal(v[12:].reshape(3, 3), Vt)
            assert np.allclose(w, np.linalg.svd(A)[1], atol=1e-13) and w[0] >= w[1] >= w[2]
            assert np.allclose(U.T @ U, np.eye(3), atol=1e-12) and np.allclose(Vt @ Vt.T, np.eye(3), atol=1e-12)
            if rank3:
                assert np.allclose(U @ np.diag(w) @ Vt, A, atol=1e-13)
            else:
                assert np.allclose(U[:, :2] @ np.diag(w[:2]) @ Vt[:2], A, atol=1e-13)


def test_rule_matches_the_reference_over_the_full_product(exe):
    """hs_twoview_rule.h against ReconstructF's / ReconstructH's control flow (twoview_ref.rule_f / rule_h restate it
    branch by branch): counts around every threshold (50, 0.9 N, 0.7 and 0.75 of the best), equal counts, and the
    parallax below, at and above minParallax."""
    down = np.nextafter(f32(1), f32(0))
    up = np.nextafter(f32(1), f32(2))
    cases = []
    vals_f = [0, 35, 50, 51, 70, 71, 100]                 # 70 = 0.7 * 100, 50 = minTriangulated
    pars_f = [(down,) * 4, (f32(1),) * 4, (up,) * 4, (up, down, up, down), (down, up, down, up)]
    for g in itertools.product(vals_f, repeat=4):
        for p in pars_f:
            for N in (40, 56, 57, 111, 112):              # int(0.9 * 56) = 50, int(0.9 * 112) = 100
                cases.append((1, N, g + (0,) * 4, p + (f32(0),) * 4))
    vals_h = [0, 51, 74, 75, 100]
    for g in itertools.product(vals_h, vals_h, vals_h, [0, 75, 100], [0, 100], [0, 74], [0, 50], [0, 100]):
        for p in ((down,) * 8, (f32(1),) * 8, (up, down) * 4):
            for N in (56, 111, 112):                      # 0.9 * 111 = 99.9 < 100 <= 0.9 * 112
                cases.append((0, N, g, p))
    text = "".join(f"{m} {N} " + " ".join(map(str, g)) + " " + " ".join(f"{bits(x):x}" for x in p) + "\n"
                   for m, N, g, p in cases)
    rows = run(exe, "rule", text)
    assert len(rows) == len(cases)
    seen = set()
    for (m, N, g, p), r in zip(cases, rows):
        want = (tr.rule_f if m else tr.rule_h)(list(g), list(p), N)
        assert tuple(map(int, r)) == want, (m, N, g, p, r, want)
        seen.add((m, want[0], want[1]))
    assert seen == {(m, 1, 0) for m in (0, 1)} | {(m, 0, w) for m in (0, 1) for w in (3, 4)}


# ---- 3. the spread of the model itself

def null_svd(A):
    return np.array([np.linalg.svd(a)[2][8] for a in A])


def null_eig(A):
    return np.array([np.linalg.eigh(a.T @ a)[1][:, 0] for a in A])


def model_spread(kind, n, ns):
    """(the largest entry-wise difference between the fp32 hypothesis matrices built from the SVD of A and from the
    eigenvector of A^T A, unit norm and one sign; which sets have a defined null vector, for H and for F)."""
    s = tc.scene(kind, n)
    sets = tc.sets_of(kind, n, ns)
    AH, AF = tr.design_matrices(s["xy1"], s["xy2"], sets)[:2]
    defined = []
    for A in (AH, AF):
        sv = np.linalg.svd(A, compute_uv=False)
        defined.append(sv[:, 7] > 1e-6 * sv[:, 0])
    a = tr.hypotheses(s["xy1"], s["xy2"], sets, null=null_svd)
    b = tr.hypotheses(s["xy1"], s["xy2"], sets, null=null_eig)
    dh = np.abs(canon(a[0]) - canon(b[0], a[0])).max(axis=1)
    df = np.abs(canon(a[2]) - canon(b[2], a[2])).max(axis=1)
    worst = max(dh[defined[0]].max(initial=0.0), df[defined[1]].max(initial=0.0))
    return float(worst), defined[0], defined[1]


SPREAD_CASES = [("general", 67, 200), ("general", 300, 200), ("general", 2049, 200), ("planar", 67, 200),
                ("planar", 300, 200), ("planar", 2049, 200)]


def test_spread_of_the_model():
    """Printed, and recorded in DESIGN.md §4: what two fp64 routes to the same hypothesis matrix differ by after the
    rounding to fp32.  tests/test_gpu_twoview.py takes 4 x this number (floor 2^-22) as its bar."""
    worst = 0.0
    for kind, n, ns in SPREAD_CASES:
        sp, dh, df = model_spread(kind, n, ns)
        print(f"{kind} n={n}: spread {sp:.3e}, undefined sets H {int((~dh).sum())} F {int((~df).sum())} of {ns}")
        assert (~dh).mean() <= 0.05 and (~df).mean() <= 0.05
        worst = max(worst, sp)
    print(f"model spread over all cases: {worst:.3e}")
    assert 0 < worst < 1e-4
    # the model's own Jacobi lies inside the same spread
    for kind, n, ns in SPREAD_CASES[:2]:
        s = tc.scene(kind, n)
        sets = tc.sets_of(kind, n, ns)
        sp, dh, df = model_spread(kind, n, ns)
        a = tr.hypotheses(s["xy1"], s["xy2"], sets)
        b = tr.hypotheses(s["xy1"], s["xy2"], sets, null=null_svd)
        bar = max(4 * sp, 2.0 ** -22)
        assert np.abs(canon(a[0]) - canon(b[0], a[0])).max(axis=1)[dh].max() <= bar
        assert np.abs(canon(a[2]) - canon(b[2], a[2])).max(axis=1)[df].max() <= bar
