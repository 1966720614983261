"""Initializer::FindTransformation (Src/Initializer.cpp:401-455) on the device through include/hs_twoview.h: the
8-point H / F hypotheses of the caller's mvSets, their scores, the model choice, the 4 or 8 motion hypotheses, CheckRT,
the decision and the median-depth scaling.  The sets are the caller's (draw_sets restates the reference's loop over a
numpy generator) or drawn on the device from the context's own cv::RNG-style generator (fit_flow_drawn).

    tv = TwoViewFit(capacity, (fx, fy, cx, cy))
    sets = draw_sets(200, status, np.random.default_rng(0))
    res = tv.fit(xy1, xy2, status, sets)            # host arrays; or
    res = tv.fit_flow(flow, sets)                   # FirstFramePts / MatchedPts / MatchedStatus where the flow holds them
    tv.rng_skip(3 * nFeatures)                      # ColorVec's draws of a first frame
    res = tv.fit_flow_drawn(flow, 200)              # the same with mvSets drawn on the device; tv.sets() reads them
    if res.ok: R, t = res.R, res.t                  # t already divided by the median depth
    g = tv.get()                                    # dict(inliers_h, inliers_f, scores_h, scores_f, triangulated, p3d, models)
    refiner.set_points_twoview(flow, tv)            # vbTriangulated and z, device to device
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, load, ptr

MAX_SETS = 256


class TwoViewResult(C.Structure):
    _fields_ = [("ok", C.c_int32), ("why", C.c_int32), ("model", C.c_int32), ("best_h", C.c_int32),
                ("best_f", C.c_int32), ("n_inliers", C.c_int32), ("SH", C.c_float), ("SF", C.c_float),
                ("_R", C.c_float * 9), ("_t", C.c_float * 3), ("n_good", C.c_int32), ("parallax_deg", C.c_float),
                ("n_triangulated", C.c_int32), ("median_depth", C.c_float), ("best_rt", C.c_int32),
                ("n_rt", C.c_int32), ("reserved", C.c_int32 * 6)]

    @property
    def R(self):
        return np.array(self._R, np.float32).reshape(3, 3)

    @property
    def t(self):
        return np.array(self._t, np.float32)

    def astuple(self):
        """Every field as bytes-comparable values (the determinism tests compare two of these)."""
        return bytes(self)


assert C.sizeof(TwoViewResult) == 128


def draw_sets(n_sets: int, status, rng) -> np.ndarray:
    """mvSets (Src/Initializer.cpp:404-432) over a numpy generator instead of cv::RNG: for every set, 8 draws without
    replacement from the keys with status != 0 by the reference's swap-and-pop (the drawn slot takes the last
    available index, the list shrinks by one)."""
    all_idx = [int(i) for i in np.flatnonzero(np.asarray(status) != 0)]
    if len(all_idx) < 8:
        raise ValueError("fewer than 8 keys with status != 0")
    sets = np.zeros((n_sets, 8), np.int32)
    for it in range(n_sets):
        avail = list(all_idx)
        for j in range(8):
            # randomGen->uniform(0, size - 1): cv::RNG's upper bound is exclusive, so the last slot is never drawn
            # directly (it moves into the drawn slot); uniform(0, 0) is 0
            hi = len(avail) - 1
            r = int(rng.integers(0, hi)) if hi > 0 else 0
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


class TwoViewFit:
    def __init__(self, capacity: int, K4, device: int = 0):
        self.lib = load()
        self.capacity = int(capacity)
        self.n = 0
        self.n_sets = (0, 0)
        self.n_fit_sets = 0
        k = (C.c_double * 4)(*[float(x) for x in K4])
        h = C.c_void_p()
        check(self.lib.hs_twoview_create(C.byref(h), device, self.capacity, k))
        self.h = h

    @classmethod
    def create(cls, capacity: int, K4, device: int = 0):
        return cls(capacity, K4, device)

    def close(self):
        if getattr(self, "h", None):
            self.lib.hs_twoview_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    @staticmethod
    def _sets(sets):
        s = np.ascontiguousarray(sets, np.int32)
        if s.ndim != 2 or s.shape[1] != 8:
            raise ValueError(f"sets must be (n_sets, 8), got {s.shape}")
        return s

    def fit(self, xy1, xy2, status, sets) -> TwoViewResult:
        """One FindTransformation on host arrays: xy1 = FirstFramePts, xy2 = MatchedPts (n, 2), status =
        MatchedStatus (n,), sets = mvSets (n_sets, 8)."""
        a = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
        st = np.ascontiguousarray(status, np.uint8)
        if len(b) != len(a) or len(st) != len(a):
            raise ValueError("xy1, xy2 and status differ in length")
        s = self._sets(sets)
        res = TwoViewResult()
        check(self.lib.hs_twoview_fit(self.h, len(a), ptr(a), ptr(b), ptr(st), len(s), ptr(s), C.byref(res)))
        self.n, self.n_sets, self.n_fit_sets = len(a), (len(s), len(s)), len(s)
        return res

    def fit_flow(self, flow, sets) -> TwoViewResult:
        """The same with the keys read on the device where a hslam_amd.flow.KeypointFlow holds them after a track."""
        s = self._sets(sets)
        res = TwoViewResult()
        n = C.c_int()
        check(self.lib.hs_flow_get(flow.h, C.byref(n), *([None] * 6)))
        check(self.lib.hs_twoview_fit_flow(self.h, flow.h, len(s), ptr(s), C.byref(res)))
        self.n, self.n_sets, self.n_fit_sets = n.value, (len(s), len(s)), len(s)
        return res

    def rng_seed(self, seed: int = 0):
        """cv::RNG(seed): a seed of 0 becomes 0xffffffff.  A new TwoViewFit is seeded with 0."""
        check(self.lib.hs_twoview_rng_seed(self.h, int(seed)))

    def rng_skip(self, n_next: int):
        """n_next draws thrown away (ColorVec takes 3 * nFeatures at every first frame)."""
        check(self.lib.hs_twoview_rng_skip(self.h, int(n_next)))

    def rng_state(self) -> int:
        st = C.c_uint64()
        check(self.lib.hs_twoview_rng_state(self.h, C.byref(st)))
        return int(st.value)

    def draw(self, status, n_sets: int):
        """Parity entry: (mvSets (n_sets, 8) int32, m) drawn on the device over a host status array; advances the
        generator."""
        st = np.ascontiguousarray(status, np.uint8)
        sets = np.zeros((max(int(n_sets), 1), 8), np.int32)
        m = C.c_int()
        check(self.lib.hs_twoview_draw(self.h, len(st), ptr(st), int(n_sets), ptr(sets), C.byref(m)))
        return sets[:int(n_sets)].copy(), m.value

    def fit_flow_drawn(self, flow, n_sets: int = 200) -> TwoViewResult:
        """fit_flow with mvSets drawn on the device from the flow's MatchedStatus.  Fewer than 8 matched keys: ok 0,
        why 5, the generator does not move.  reserved[0], reserved[1] of the record are the generator's state."""
        res = TwoViewResult()
        n = C.c_int()
        check(self.lib.hs_flow_get(flow.h, C.byref(n), *([None] * 6)))
        check(self.lib.hs_twoview_fit_flow_drawn(self.h, flow.h, int(n_sets), C.byref(res)))
        if res.why != 5:
            self.n, self.n_sets, self.n_fit_sets = n.value, (int(n_sets), int(n_sets)), int(n_sets)
        return res

    def sets(self) -> np.ndarray:
        """mvSets of the last fit, drawn or uploaded: (n_sets, 8) int32."""
        s = np.zeros((self.n_fit_sets, 8), np.int32)
        check(self.lib.hs_twoview_get_sets(self.h, ptr(s)))
        return s

    def last_draw_stats(self):
        """Device ms of the last draw's kernels: good_list, draw."""
        ms = (C.c_double * 2)()
        check(self.lib.hs_twoview_last_draw_stats(self.h, ms))
        return dict(good_list=float(ms[0]), draw=float(ms[1]))

    def last_result(self) -> TwoViewResult:
        res = TwoViewResult()
        check(self.lib.hs_twoview_last_result(self.h, C.byref(res)))
        return res

    def get(self):
        """dict(inliers_h, inliers_f (n,) uint8; scores_h (n_h,), scores_f (n_f,) float32; triangulated (n,) uint8; p3d
        (n, 3) float32, divided by the median depth; models_h (n_h, 3, 3), models_f (n_f, 3, 3) float32) of the last
        fit or debug entry."""
        n, (nh, nf) = self.n, self.n_sets
        o = dict(inliers_h=np.zeros(n, np.uint8), inliers_f=np.zeros(n, np.uint8), scores_h=np.zeros(nh, np.float32),
                 scores_f=np.zeros(nf, np.float32), triangulated=np.zeros(n, np.uint8), p3d=np.zeros((n, 3), np.float32))
        models = np.zeros((nh + nf, 3, 3), np.float32)
        check(self.lib.hs_twoview_get(self.h, ptr(o["inliers_h"]), ptr(o["inliers_f"]), ptr(o["scores_h"]),
                                      ptr(o["scores_f"]), ptr(o["triangulated"]), ptr(o["p3d"]), ptr(models)))
        o["models_h"], o["models_f"] = models[:nh].copy(), models[nh:].copy()
        return o

    def get_rt(self):
        """CheckRT per motion hypothesis: dict(n_good (n_rt,), parallax (n_rt,), good, passed (n_rt, n) uint8,
        cos_parallax (n_rt, n), p3d (n_rt, n, 3))."""
        k = C.c_int()
        check(self.lib.hs_twoview_get_rt(self.h, C.byref(k), *([None] * 6)))
        m, n = k.value, self.n
        o = dict(n_good=np.zeros(m, np.int32), parallax=np.zeros(m, np.float32), good=np.zeros((m, n), np.uint8),
                 passed=np.zeros((m, n), np.uint8), cos_parallax=np.zeros((m, n), np.float32),
                 p3d=np.zeros((m, n, 3), np.float32))
        check(self.lib.hs_twoview_get_rt(self.h, None, ptr(o["n_good"]), ptr(o["parallax"]), ptr(o["good"]),
                                         ptr(o["passed"]), ptr(o["cos_parallax"]), ptr(o["p3d"])))
        return o

    def last_stats(self):
        """Device ms of the last fit's kernels: normalize, hypotheses, scores, winners, decompose, check_rt, select,
        finish."""
        ms = (C.c_double * 8)()
        check(self.lib.hs_twoview_last_stats(self.h, ms))
        return dict(zip(("normalize", "hypotheses", "scores", "winners", "decompose", "check_rt", "select", "finish"),
                        [float(x) for x in ms]))

    def score_models(self, H21, H12, F21):
        """Debug: only the scoring of caller-supplied fp32 matrices on the keys of the last fit; read with get()."""
        h = np.ascontiguousarray(H21, np.float32).reshape(-1, 9)
        hi = np.ascontiguousarray(H12, np.float32).reshape(-1, 9)
        f = np.ascontiguousarray(F21, np.float32).reshape(-1, 9)
        if len(hi) != len(h):
            raise ValueError("H21 and H12 differ in length")
        check(self.lib.hs_twoview_score_models(self.h, len(h), ptr(h), ptr(hi), len(f), ptr(f)))
        self.n_sets = (len(h), len(f))

    def check_rt(self, R, t, inliers):
        """Debug: only CheckRT of caller-supplied motions over the matches with inliers != 0; read with get_rt()."""
        r = np.ascontiguousarray(R, np.float32).reshape(-1, 9)
        tt = np.ascontiguousarray(t, np.float32).reshape(-1, 3)
        m = np.ascontiguousarray(inliers, np.uint8)
        if len(tt) != len(r) or len(m) != self.n:
            raise ValueError("R, t or inliers have the wrong length")
        check(self.lib.hs_twoview_check_rt(self.h, len(r), ptr(r), ptr(tt), ptr(m)))
