"""The frame rule of hs_ba_flag_frames_for_marginalization on the host (hs_debug_frame_rule calls the same inline the
kernel calls, hs_frame_rule.h) against a numpy restatement of System::flagFramesForMarginalization
(Src/FullSystemMarginalize.cpp:18-103; tests/map_ref.py) over a planted product.  Every planted value is well away from
its threshold (|log affine factor| at least 0.05 from 0.7, the two smallest distance scores at least 1e-3 apart,
relative), so that neither logf's rounding nor the sum's can flip a decision.  No GPU needed."""
import ctypes as C
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-slam_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import map_ref  # noqa: E402
from map_ref import WHY_AFFINE, WHY_AGE, WHY_BLOCKED, WHY_POINTS, WHY_SCORE  # noqa: E402

# camera positions along a line (irregular steps, so that no two distance scores tie), two geometries
GEOMETRY = [np.cumsum([0.0, 0.06, 0.09, 0.05, 0.12, 0.07, 0.10, 0.08]),
            np.cumsum([0.0, 0.20, 0.03, 0.04, 0.05, 0.30, 0.06, 0.02])]
FEW = [(), (1,), (0, 2), (1, 2, 3, 4)]            # frames under the 5 % rule
AFF = [(), (2,), (1, 3), (0, 1, 2, 3)]            # frames over the affine bar
KFID = ["from0", "from3", "gapped"]
PARAMS = [dict(), dict(minFrameAge=3), dict(minFrameAge=7), dict(minFrameAge=8), dict(maxFrames=5, minFrameAge=6),
          dict(maxFrames=6, minFrames=3)]
LOG_OVER = [0.9, -0.75, 0.76, -1.3]               # |log| >= 0.75
LOG_UNDER = [0.0, 0.3, -0.65, 0.64, -0.1, 0.2, -0.4, 0.5]


def _case(nF, geo, few, aff, kfid, over):
    from hslam_amd.map import frame_marg_params
    P = frame_marg_params(**over)
    x = GEOMETRY[geo][:nF]
    dist = np.abs(x[:, None] - x[None, :]).astype(np.float32)
    n_in = np.array([80, 6, 0, 40, 80, 7, 33, 80][:nF], np.int32)
    n_out = np.array([100, 100, 0, 0, 20, 100, 5, 100][:nF], np.int32)
    logs = np.array(LOG_UNDER[:nF])
    for f in few:
        if f < nF:
            n_in[f], n_out[f] = 2, 100
    for i, f in enumerate(aff):
        if f < nF:
            logs[f] = LOG_OVER[i]
    aff0 = np.exp(logs)
    kf = dict(from0=np.arange(nF), from3=np.arange(nF) + 3, gapped=np.cumsum([1, 2, 1, 3, 1, 1, 2, 1])[:nF])[kfid]
    return P, n_in, n_out, aff0, dist, kf.astype(np.int32)


def test_frame_rule_matches_the_reference_over_the_planted_product():
    from hslam_amd import _lib
    fn = _lib.load().hs_debug_frame_rule
    seen = dict(why=set(), both=0, empty=0, none=0, sizes={}, score_ran=0, kf0_excluded=0, age_excluded=0, cases=0)
    for nF, geo, few, aff, kfid, over in itertools.product(range(4, 9), range(2), FEW, AFF, KFID, PARAMS):
        P, n_in, n_out, aff0, dist, kf = _case(nF, geo, few, aff, kfid, over)
        # the plants keep their distance from the thresholds
        lg = np.log(aff0)
        assert (np.abs(np.abs(lg) - 0.7) >= 0.05 - 1e-12).all()
        want, why = map_ref.frame_rule(n_in, n_out, aff0, dist, kf, P)
        if P.minFrameAge <= P.maxFrames and nF - int(((why & (WHY_POINTS | WHY_AFFINE)) != 0).sum()) >= P.maxFrames:
            sc = map_ref.frame_scores(dist, kf, P.minFrameAge)
            live = sorted(s for s in sc if s is not None)
            seen["score_ran"] += 1
            if not live:
                seen["empty"] += 1
                assert not (why & WHY_SCORE).any()
            else:
                assert live[0] < 1
                if len(live) > 1:
                    assert (live[1] - live[0]) >= 1e-3 * abs(live[0]), (nF, geo, kfid, over, live[:2])
                pick = int(np.nonzero(why & WHY_SCORE)[0][0])
                # both exclusions occur among the frames that would otherwise have a score
                unfiltered = map_ref.frame_scores(dist, np.arange(nF) + 100, 0)  # every frame passes
                for f in range(nF):
                    if sc[f] is None and unfiltered[f] is not None:
                        seen["kf0_excluded" if kf[f] == 0 else "age_excluded"] += 1
                assert sc[pick] == live[0]
        got = np.zeros(nF, np.uint8)
        gwhy = np.zeros(nF, np.uint8)
        n = fn(nF, _lib.ptr(n_in), _lib.ptr(n_out), _lib.ptr(aff0), _lib.ptr(dist), _lib.ptr(kf), C.addressof(P),
               _lib.ptr(got), _lib.ptr(gwhy))
        assert np.array_equal(got, want), (nF, geo, few, aff, kfid, over, got, want)
        assert np.array_equal(gwhy, why), (nF, geo, few, aff, kfid, over, gwhy, why)
        assert n == int(want.sum())
        seen["cases"] += 1
        seen["why"] |= set(int(w) for w in why)
        seen["both"] += int(((why & 3) == 3).sum())
        seen["none"] += int(want.sum() == 0)
        seen["sizes"].setdefault(nF, set()).add(int(want.sum()))
    print({k: (sorted(v) if isinstance(v, set) else v) for k, v in seen.items()})
    bits = 0
    for w in seen["why"]:
        bits |= w
    assert bits == WHY_POINTS | WHY_AFFINE | WHY_SCORE | WHY_AGE | WHY_BLOCKED
    assert seen["both"] > 0 and seen["empty"] > 0 and seen["none"] > 0 and seen["score_ran"] > seen["empty"]
    assert seen["kf0_excluded"] > 0 and seen["age_excluded"] > 0
    # below minFrames nothing can be flagged by the clauses; every larger window has flagged and unflagged cases
    assert all(len(seen["sizes"][nF]) > 1 for nF in range(5, 9))


def test_ctypes_structs_match_c_layout(tmp_path):
    """hs_map_record is 64 bytes and the ctypes / numpy mirrors of include/hs_map.h have the C structs' sizes."""
    import subprocess
    from hslam_amd import _lib
    from hslam_amd.map import RECORD
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "hs_map.h"\n'
                   'int main(void){printf("%zu %zu\\n", sizeof(hs_map_record), sizeof(hs_frame_marg_params));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert sizes == [64, 20]
    assert [C.sizeof(_lib.hs_map_record), C.sizeof(_lib.hs_frame_marg_params)] == sizes and RECORD.itemsize == 64
    assert [RECORD.fields[n][1] for n in ("handle", "u", "hdif", "color", "reserved")] == [0, 16, 32, 40, 48]
    assert _lib.hs_map_record.color.offset == 40 and _lib.hs_map_record.hdif.offset == 32


def test_named_windows():
    """The issue's planted windows one by one, with the reference's settings."""
    from hslam_amd import _lib
    from hslam_amd.map import frame_marg_params
    fn = _lib.load().hs_debug_frame_rule

    def run(nF, few=(), aff=(), kfid="from3", **over):
        P, n_in, n_out, aff0, dist, kf = _case(nF, 0, few, aff, kfid, over)
        got, why = np.zeros(nF, np.uint8), np.zeros(nF, np.uint8)
        fn(nF, _lib.ptr(n_in), _lib.ptr(n_out), _lib.ptr(aff0), _lib.ptr(dist), _lib.ptr(kf), C.addressof(P),
           _lib.ptr(got), _lib.ptr(why))
        want, wwhy = map_ref.frame_rule(n_in, n_out, aff0, dist, kf, P)
        assert np.array_equal(got, want) and np.array_equal(why, wwhy)
        return got, why

    P = frame_marg_params()
    assert (P.minFrameAge, P.maxFrames, P.minFrames) == (1, 7, 5)
    assert abs(P.minPointsRemaining - 0.05) < 1e-8 and abs(P.maxLogAffFacInWindow - 0.7) < 1e-7
    # below minFrames: the clauses hold and are blocked, and 4 < maxFrames runs no score
    got, why = run(4, few=(1,), aff=(2,))
    assert not got.any() and why[1] == WHY_BLOCKED and why[2] == WHY_BLOCKED
    # between: 6 frames, the first clause flags (6 > 5), the second is blocked (5 > 5 fails)
    got, why = run(6, few=(1,), aff=(2,))
    assert got.tolist() == [0, 1, 0, 0, 0, 0] and why[1] == WHY_POINTS and why[2] == WHY_BLOCKED
    got, why = run(6, aff=(2,))
    assert got.tolist() == [0, 0, 1, 0, 0, 0] and why[2] == WHY_AFFINE
    # at maxFrames without a clause: the distance score flags exactly one
    got, why = run(7)
    assert got.sum() == 1 and (why == WHY_SCORE).sum() == 1 and not got[-1]
    # both clauses at once; size - flagged reaches minFrames after three flags, the fourth is blocked
    got, why = run(8, few=(1, 2, 3, 4), aff=(2,))
    assert got.tolist() == [0, 1, 1, 1, 0, 0, 0, 0] and why[2] == (WHY_POINTS | WHY_AFFINE) and why[4] == WHY_BLOCKED
    # KfId == 0 and the age exclusion: frame 0 (KfId 0) and the newest never take the score flag
    for age in (1, 3):
        got, why = run(7, kfid="from0", minFrameAge=age)
        pick = int(np.nonzero(got)[0][0])
        assert got.sum() == 1 and pick != 0 and pick <= 6 - age
    # no frame passes the age test: nothing is flagged (the reference would dereference an empty toMarginalize)
    got, why = run(7, minFrameAge=7)
    assert not got.any() and not why.any()
    # minFrameAge > maxFrames: the early branch flags frames [0, size - maxFrames)
    got, why = run(8, minFrameAge=8)
    assert got.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and why[0] == WHY_AGE
    got, why = run(8, maxFrames=5, minFrameAge=6)
    assert got.tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
