"""The initializer's generator, draw and decision table without a GPU: the model of include/hs_twoview.h's "Generator"
and "Draw of mvSets" (tests/initializer_ref.py) against known answers and against the existing restatement of the draw
(hslam_amd.twoview.draw_sets), the exported entries, and hslam_amd.initializer.decide row by row."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "h-slam_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from initializer_ref import CvRng, draw_sets_cv  # noqa: E402
from hslam_amd.twoview import draw_sets  # noqa: E402

ENTRIES = {"hs_twoview.h": ["hs_twoview_rng_seed", "hs_twoview_rng_skip", "hs_twoview_rng_state", "hs_twoview_draw",
                            "hs_twoview_fit_flow_drawn", "hs_twoview_get_sets"],
           "hs_flow.h": ["hs_flow_mean_flow_device"]}


# ---- the generator

def test_known_answers_from_seed_0():
    r = CvRng(0)
    assert r.state == 0xFFFFFFFF
    assert [r.next() for _ in range(4)] == [0x07C09CF6, 0xB302A6A5, 0xE6ABD4E7, 0x507B8A5D]
    assert r.state == 0xDFAF93C7507B8A5D
    assert CvRng(5).state == 5 and CvRng(1 << 40).state == 1 << 40


def test_uniform_bounds_and_the_draw_it_does_not_take():
    r = CvRng(0)
    before = r.state
    assert r.uniform(0, 0) == 0 and r.uniform(7, 7) == 7 and r.state == before     # a == b consumes nothing
    q = CvRng(0)
    assert r.uniform(0, 1) == 0 and r.state != before                             # b is exclusive: [0, 1) is 0
    assert r.state == (q.next(), q.state)[1]                                      # and one draw was taken
    vals = [r.uniform(3, 6) for _ in range(400)]
    assert set(vals) == {3, 4, 5}
    a, b = CvRng(9), CvRng(9)
    assert [a.uniform(0, 255) for _ in range(50)] == [b.next() % 255 for _ in range(50)]


def test_skip_is_that_many_next():
    a, b = CvRng(3), CvRng(3)
    a.skip(6000)
    for _ in range(6000):
        b.next()
    assert a.state == b.state


# ---- the draw

class Shim:
    """A numpy-generator look-alike over CvRng: integers(0, hi) = next() % hi, which is uniform(0, hi) for hi > 0."""
    def __init__(self, rng):
        self.rng = rng

    def integers(self, lo, hi):
        assert lo == 0 and hi > 0
        return self.rng.next() % hi


def status_of(n, bad, seed=1):
    st = np.ones(n, np.uint8)
    st[np.random.default_rng(seed).choice(n, bad, replace=False)] = 0
    return st


@pytest.mark.parametrize("n, bad, n_sets", [(8, 0, 3), (9, 1, 5), (9, 0, 5), (67, 5, 200), (300, 40, 200),
                                            (2049, 205, 256)])
def test_draw_equals_the_existing_restatement(n, bad, n_sets):
    st = status_of(n, bad)
    a, b = CvRng(0), CvRng(0)
    sets = draw_sets_cv(st, n_sets, a)
    want = draw_sets(n_sets, st, Shim(b))
    assert np.array_equal(sets, want) and a.state == b.state
    assert sets.shape == (n_sets, 8) and sets.dtype == np.int32
    for s in sets:                                                   # 8 distinct good keys
        assert len(set(s.tolist())) == 8 and st[s].all()
    m = int(st.sum())
    c = CvRng(0)
    c.skip(n_sets * (7 if m == 8 else 8))                            # m == 8: the eighth draw is uniform(0, 0)
    assert a.state == c.state


def test_the_draw_runs_on_across_calls():
    st = status_of(67, 5)
    a, b = CvRng(0), CvRng(0)
    one = draw_sets_cv(st, 10, a)
    two = np.concatenate([draw_sets_cv(st, 4, b), draw_sets_cv(st, 6, b)])
    assert np.array_equal(one, two) and a.state == b.state
    with pytest.raises(ValueError):
        draw_sets_cv(status_of(9, 2), 1, a)
    assert a.state == b.state


# ---- the entries

def test_the_new_entries_are_declared_and_exported():
    lib = ctypes.CDLL(os.path.join(ROOT, "h-slam_amd", "lib", "libhslam_amd.so"))
    for header, names in ENTRIES.items():
        txt = open(os.path.join(ROOT, "include", header)).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        for name in names:
            assert re.search(r"^int\s+%s\s*\(" % name, txt, flags=re.M), name
            assert hasattr(lib, name), name
    from hslam_amd._lib import SIGNATURES
    assert all(n in SIGNATURES for names in ENTRIES.values() for n in names)


def test_the_generator_entries_need_no_device():
    """seed / skip / state are host state of the context; a null context is refused, not dereferenced."""
    lib = ctypes.CDLL(os.path.join(ROOT, "h-slam_amd", "lib", "libhslam_amd.so"))
    st = ctypes.c_uint64()
    assert lib.hs_twoview_rng_state(None, ctypes.byref(st)) == -1
    assert lib.hs_twoview_rng_seed(None, ctypes.c_uint64(0)) == -1
    assert lib.hs_twoview_rng_skip(None, ctypes.c_uint64(1)) == -1


# ---- the decision table

def test_decision_table_row_by_row():
    from hslam_amd import initializer as ini
    d = ini.decide
    # no first frame
    assert d(False, 0, 100)[:3] == (ini.NO_FRAME, 0, False)                        # nFeatures > 100 is strict
    assert d(False, 3, 101)[:3] == (ini.FIRST, 3, True)                            # NumFails is not touched
    # NumFails > 40 at entry: reset, and the same call may take the frame as the first frame
    r = d(True, 41, 300, 300)
    assert r.action == ini.FIRST and r.num_fails == 0 and r.has_first and r.reset_at_entry
    r = d(True, 41, 50, 300)
    assert r.action == ini.NO_FRAME and r.num_fails == 0 and not r.has_first and r.reset_at_entry
    assert d(True, 40, 300, 300).action == ini.NEED_TRACK                          # > 40 is strict
    # a second frame with too few features
    assert d(True, 2, 100, 300)[:3] == (ini.RESET_FEATURES, 2, False)
    # nmatches < 0.2f * nFeatures, in float
    assert d(True, 0, 300, 300, 59)[:3] == (ini.RESET_MATCHES, 0, False)
    assert d(True, 0, 300, 300, 60).action == ini.NEED_MEAN_FLOW                   # (float)60 < 0.2f * 300.f is false
    assert d(True, 0, 300, 1385, 277).action == ini.NEED_MEAN_FLOW                 # 0.2f * 1385.f = 277.0f in float
    assert d(True, 0, 300, 1385, 276).action == ini.RESET_MATCHES
    # stationary: no reset, NumFails untouched
    r = d(True, 7, 300, 300, 200, 1.9999)
    assert r[:3] == (ini.STATIONARY, 7, True)
    assert d(True, 7, 300, 300, 200, 2.0).action == ini.NEED_FIT
    assert d(True, 7, 300, 300, 200, float("nan")).action == ini.NEED_FIT         # NaN < 2.0f is false
    # the fit refuses
    assert d(True, 7, 300, 300, 200, 3.0, (False, 0))[:3] == (ini.FIT_FAILED, 8, True)
    assert d(True, 40, 300, 300, 200, 3.0, (False, 0))[:3] == (ini.FIT_FAILED, 41, True)
    # the fit succeeds: NumFails = 0; the untriangulated keys leave nmatches
    r = d(True, 7, 300, 300, 250, 3.0, (True, 200))
    assert r == (ini.SUCCESS, 0, True, 150, False)                                 # 250 - (300 - 200)
    r = d(True, 7, 300, 300, 250, 3.0, (True, 199))
    assert r == (ini.RESET_TRIANGULATED, 0, False, 149, False)                     # < 150
    r = d(True, 7, 2000, 2000, 1000, 3.0, (True, 1199))
    assert r[:4] == (ini.RESET_TRIANGULATED, 0, False, 199)                        # < 0.1 * 2000
    assert d(True, 7, 2000, 2000, 1000, 3.0, (True, 1200)).action == ini.SUCCESS
