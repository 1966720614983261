"""The per-point rule of hs_ba_flag_points_for_removal on the host (hs_debug_flag_rule calls the same inline the
kernel calls) against a numpy restatement of System::flagPointsForRemoval (Src/Mapping.cpp:248-328) with
MapPoint::isOOB / isInlierNew (Include/MapPoint.h:133-161).  No GPU needed."""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-slam_amd"))

IN, OOB, OUT = 0, 1, 2


def reference_rule(nres, vis, n_good, idepth, hdif, last0, last1, host_flagged):
    """(action, flag_nores, flag_oob, flag_in, flag_inin) arrays, the reference's control flow branch by branch.
    Settings.cpp:96,97,119: minGoodActiveResForMarg 3, minGoodResForMarg 4, minIdepthH_marg 50."""
    n = len(nres)
    action = np.zeros(n, np.int64)
    cnt = np.zeros((n, 4), np.int64)
    for i in range(n):
        if idepth[i] < 0 or nres[i] == 0:           # Mapping.cpp:268: toDrop, flag_nores++
            action[i], cnt[i, 0] = 1, 1
            continue
        # MapPoint::isOOB
        is_oob = False
        if nres[i] >= 3 and n_good[i] > 4 + 10 and nres[i] - vis[i] < 3:
            is_oob = True
        elif last0[i] == OOB:
            is_oob = True
        elif nres[i] < 2:
            is_oob = False
        elif last0[i] == OUT and last1[i] == OUT:
            is_oob = True
        if not (is_oob or host_flagged[i]):
            continue
        cnt[i, 1] = 1                                # flag_oob++
        if nres[i] >= 3 and n_good[i] >= 4:          # isInlierNew
            cnt[i, 2] = 1                            # flag_in++
            # idepth_hessian = 1 / HdiF of the last solve, in fp64 (0 when HdiF is 0: before any solve)
            h = np.float64(np.float32(hdif[i]))
            idepth_hessian = 1.0 / h if h > 0 else 0.0
            if idepth_hessian > 50.0:
                cnt[i, 3] = 1                        # flag_inin++
                action[i] = 2                        # toMarg
            else:
                action[i] = 1
        else:
            action[i] = 1
    return action, cnt


def test_flag_rule_matches_the_reference_over_the_full_product():
    from hslam_amd import _lib
    fn = _lib.load().hs_debug_flag_rule
    cases = []
    for nres in range(8):
        for vis in range(nres + 1):
            cases += [(nres, vis) + t for t in itertools.product(
                (0, 3, 4, 14, 15), (-1.0, 1.0), (0.0, 1.0 / 49.0, 1.0 / 51.0, 1e-6), (IN, OOB, OUT), (IN, OOB, OUT),
                (0, 1))]
    assert len(cases) == 36 * 5 * 2 * 4 * 3 * 3 * 2
    cols = list(zip(*cases))
    action, cnt = reference_rule(*cols)
    got = np.array([fn(*c) for c in cases], np.int64)
    assert np.array_equal(got & 3, action)
    for k, bit in enumerate((4, 8, 16, 32)):
        assert np.array_equal((got & bit) != 0, cnt[:, k] != 0), bit
    assert not np.any(got & ~63)
    # every outcome and every counter occurs, on both sides of each test
    assert set(action) == {0, 1, 2} and cnt.min(0).tolist() == [0] * 4 and cnt.max(0).tolist() == [1] * 4
