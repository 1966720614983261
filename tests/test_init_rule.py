"""The per-key rule of hs_refiner_seed_ba on the host: tests/c/init_rule_main.cpp runs h-slam_amd/csrc/hs_init_rule.h
(the inline hs_k_init_seed calls) over the full product of its inputs, against a numpy restatement of
Initializer::videpth (Src/Initializer.cpp:155-159, DirectRefinement's write-back :1393-1397) and of
System::InitFromInitializer's skips (Src/System.cpp:265-290) with the documented border deviation.  Also the mirror
guard: activation's mirror rule with empty IN masks is hs_ba_insert_points'.  No GPU needed."""
import itertools
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-slam_amd"))

W, H = 160, 120


def reference(tri, good, idepth, invz, fin, x, y):
    """(videpth, why): the reference's control flow, branch by branch."""
    # Initializer.cpp:155-159: videpth = 1 / z where triangulated, else -1; :1393-1397: the refined idepth is written
    # back where the point is good and triangulated
    if not tri:
        videpth = np.float32(-1.0)
    elif good:
        videpth = np.float32(idepth)
    else:
        videpth = np.float32(invz)
    if videpth <= np.float32(0.0):                       # System.cpp:267 (a NaN is not <= 0: it goes on)
        return videpth, 1
    # the ImmaturePoint constructor at (x, y) = mvKeys[i].pt + 0.5f (:270-271) reads 2 px around it plus one texel:
    # where that leaves the image the reference reads outside its buffer; the port skips the key (code 3), with
    # hs_tracer_add_points' rule
    if not (x >= 2 and y >= 2 and x < W - 3 and y < H - 3):
        return videpth, 3
    if not fin:                                          # :273 / :279 energyTH not finite
        return videpth, 2
    return videpth, 0


def bits(f):
    return int(np.array([f], np.float32).view(np.uint32)[0])


def test_init_rule_matches_the_reference_over_the_full_product(tmp_path):
    exe = tmp_path / "init_rule_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "c", "init_rule_main.cpp"), "-o", str(exe)], check=True)
    f32 = np.float32
    depths = [f32(-1.5), f32(-0.0), f32(0.0), f32(0.7), f32(np.nan)]
    cx, cy = f32(80.5), f32(60.5)
    down = lambda v: np.nextafter(f32(v), f32(-np.inf))   # noqa: E731
    # the four border edges, each at its last legal and its first illegal value, and one interior position
    places = [(cx, cy),
              (f32(2), cy), (down(2), cy), (down(W - 3), cy), (f32(W - 3), cy),
              (cx, f32(2)), (cx, down(2)), (cx, down(H - 3)), (cx, f32(H - 3))]
    cases = list(itertools.product((0, 1), (0, 1), depths, depths, (0, 1), places))
    assert len(cases) == 2 * 2 * 5 * 5 * 2 * 9
    text = "".join(f"{t} {g} {bits(i):x} {bits(z):x} {c} {bits(p[0]):x} {bits(p[1]):x} {W} {H}\n"
                   for t, g, i, z, c, p in cases)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) == len(cases) + 1 and out[-1] == ""
    why = []
    for (t, g, i, z, c, p), line in zip(cases, out):
        vb, code = line.split()
        vid, want = reference(t, g, i, z, c, p[0], p[1])
        assert int(vb, 16) == bits(vid), (t, g, i, z)
        assert int(code) == want, (t, g, i, z, c, p, code, want)
        why.append(want)
    # every code occurs, and each border position decides by itself
    assert set(why) == {0, 1, 2, 3}
    legal = [reference(1, 1, f32(0.7), f32(0.7), 1, *p)[1] for p in places]
    assert legal == [0, 0, 3, 0, 3, 0, 3, 0, 3]


def test_mirror_of_points_without_residuals_is_insert_points():
    """hs::stage_activated with empty IN masks (what hs_refiner_seed_ba stages, before its lastResiduals codes) leaves
    the mirror hs_ba_insert_points leaves: no residual, lastResiduals without a target.  A guard: it passes without the
    seeding entry."""
    from hslam_amd import _lib
    lib = _lib.load()
    for nF in (1, 2, 8):
        n = 5
        host = np.arange(n, dtype=np.int32) % nF
        masks = np.zeros(n, np.uint8)
        a, b = np.zeros((n, 12), np.int32), np.zeros((n, 12), np.int32)
        _lib.check(lib.hs_debug_act_mirror(nF, n, _lib.ptr(host), _lib.ptr(masks), _lib.ptr(a), _lib.ptr(b)))
        assert np.array_equal(a, b)
        assert not a[:, 0].any() and np.all(a[:, 1:10] == -1)
