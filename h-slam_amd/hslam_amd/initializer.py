"""Initializer::Initialize (Src/Initializer.cpp:28-225) and System::InitFromInitializer over the device bricks: the
first-frame / second-frame state machine around FeatureExtractor, KeypointFlow, TwoViewFit and DirectRefinement, as
hslam_amd.keyframe.KeyframeBA mirrors AddKeyframe.  Every hand-off goes device to device; what comes back per frame is
the key count, the match count, the mean flow (4 bytes) and the fit's result record.

    ini = Initializer(W, H, K4, capacity, pattern)
    for raw in frames:
        if ini.Initialize(raw, undistorter, exposure):            # True once: FindTransformation + DirectRefinement
            break
    ini.pose, ini.videpth(), ini.result                           # Pose, videpth, the last TwoViewResult
    why, handles, firstToNew = ini.init_window(ba)                # InitFromInitializer's first frame and point loop

The decisions are one pure function, decide(), so the table is tested without a device.  Two named deviations:
NumFails is a function-local static in the reference and survives Initializer objects, here it is a member; ColorVec
is not kept, only its 3 * nFeatures draws are consumed (TwoViewFit.rng_skip).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

MAX_FAILS = 40          # NumFails > 40: start over
MIN_FEATURES = 100      # nFeatures > 100, of a first and of a second frame
MIN_TRIANGULATED = 150  # nmatches after the untriangulated keys have left
MAX_L1_ERROR = 7        # FindMatches(15, 7)
N_SETS = 200            # mMaxIterations
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)

# what decide() can answer.  The first three ask for the next measurement; the others end the call.
NEED_TRACK, NEED_MEAN_FLOW, NEED_FIT = "need_track", "need_mean_flow", "need_fit"
NO_FRAME = "no_frame"                      # no first frame and too few features: nothing happens
FIRST = "first"                            # the frame becomes the first frame
RESET_FEATURES = "reset_features"          # a second frame with nFeatures <= 100
RESET_MATCHES = "reset_matches"            # nmatches < 0.2f * nFeatures
STATIONARY = "stationary"                  # mean flow < 2: no reset, NumFails untouched
FIT_FAILED = "fit_failed"                  # FindTransformation returned false: NumFails += 1
RESET_TRIANGULATED = "reset_triangulated"  # too few triangulated matches
SUCCESS = "success"

Decision = namedtuple("Decision", "action num_fails has_first nmatches reset_at_entry")


def decide(has_first, num_fails, n_features, n_first=None, nmatches=None, mean_flow=None, fit=None) -> Decision:
    """The exits of Initialize in the reference's order.  has_first / num_fails: the state at entry; n_features: the
    frame's nFeatures; n_first: the first frame's; nmatches: FindMatches' return; mean_flow: ComputeMeanOpticalFlow;
    fit: (ok, n_triangulated) of FindTransformation.  A measurement that is not made yet is None: the answer is then
    the request for it.  Returns (action, NumFails after, whether a first frame is held after, nmatches after the
    untriangulated keys have left or as given, whether the entry reset fired)."""
    f32 = np.float32
    reset_at_entry = num_fails > MAX_FAILS
    if reset_at_entry:                                               # :34-38
        has_first, num_fails = False, 0
    if not has_first:                                                # :40-73
        took = n_features > MIN_FEATURES
        return Decision(FIRST if took else NO_FRAME, num_fails, took, nmatches, reset_at_entry)
    if not n_features > MIN_FEATURES:                                # :76-84
        return Decision(RESET_FEATURES, num_fails, False, nmatches, reset_at_entry)
    if nmatches is None:
        return Decision(NEED_TRACK, num_fails, True, None, reset_at_entry)
    if f32(nmatches) < f32(0.2) * f32(n_first):                      # :111
        return Decision(RESET_MATCHES, num_fails, False, nmatches, reset_at_entry)
    if mean_flow is None:
        return Decision(NEED_MEAN_FLOW, num_fails, True, nmatches, reset_at_entry)
    if f32(mean_flow) < f32(2.0):                                    # :117 (a NaN passes, as in the reference)
        return Decision(STATIONARY, num_fails, True, nmatches, reset_at_entry)
    if fit is None:
        return Decision(NEED_FIT, num_fails, True, nmatches, reset_at_entry)
    ok, n_triangulated = fit
    if not ok:                                                       # :214-215
        return Decision(FIT_FAILED, num_fails + 1, True, nmatches, reset_at_entry)
    nmatches = int(nmatches) - (int(n_first) - int(n_triangulated))  # :129-131
    if nmatches < 0.1 * n_first or nmatches < MIN_TRIANGULATED:      # :133
        return Decision(RESET_TRIANGULATED, 0, False, nmatches, reset_at_entry)
    return Decision(SUCCESS, 0, True, nmatches, reset_at_entry)


def pose_of(result) -> np.ndarray:
    """Pose = SE3([R | t / MedianDepth]) (:139-153) as SE3 data (qx qy qz qw tx ty tz); result.t is already divided."""
    from .scene import se3_data
    return se3_data(result.R.astype(np.float64), result.t.astype(np.float64))


class Initializer:
    def __init__(self, width: int, height: int, K4, capacity: int, pattern=None, density: float = 600,
                 n_levels: int = 4, n_sets: int = N_SETS, device: int = 0):
        """capacity: the most keys of a frame.  pattern: the extractor's 256 x 2 x 2 test pattern; without one every
        Initialize call must bring its keys.  density: the selector's desired density of Frame::Extract."""
        from .flow import KeypointFlow
        from .image import DeviceImage
        from .refine import DirectRefinement
        from .twoview import TwoViewFit
        self.W, self.H, self.K4 = int(width), int(height), np.asarray(K4, np.float64)
        self.capacity, self.density, self.n_sets = int(capacity), float(density), int(n_sets)
        self.first_image = DeviceImage(self.W, self.H, n_levels, device)    # the candidate first frame's
        self.image = DeviceImage(self.W, self.H, n_levels, device)          # the current frame's
        self.selector = self.extractor = None
        if pattern is not None:
            from .extract import FeatureExtractor
            from .select import PixelSelector
            self.selector = PixelSelector(self.W, self.H, device=device)
            self.extractor = FeatureExtractor(self.W, self.H, self.capacity, pattern, device)
        self.flow = KeypointFlow(self.W, self.H, self.capacity, device)
        self.twoview = TwoViewFit(max(self.capacity, 8), self.K4, device)
        self.refiner = DirectRefinement.bare(self.W, self.H, self.K4, device)
        self.has_first, self.NumFails, self.n_first, self.first_exposure = False, 0, 0, 1.0
        self.n_frames = 0
        self.pose = self.result = self.good = None
        self.refine_stats = None
        self.history = []

    def close(self):
        for o in (self.first_image, self.image, self.extractor, self.flow, self.twoview, self.refiner):
            if o is not None:
                o.close()
        self.selector = None                                         # a PixelSelector frees itself when it is dropped

    def reset_rng(self, seed: int = 0):
        self.twoview.rng_seed(seed)

    def videpth(self):
        """Initializer::videpth after a success, the refinement's write-back applied."""
        return self.refiner.videpth()

    def _take_first(self, keys, n, exposure):
        """:44-58: TransitImage, FirstFramePts, mvbPrevMatched, and ColorVec's draws."""
        if keys is None:
            assert self.flow.set_first_extracted(self.extractor) == n
        else:
            self.flow.set_first_image(self.image, keys)
        self.refiner.set_first_image(self.image, exposure)
        self.first_image, self.image = self.image, self.first_image
        self.n_first, self.first_exposure = n, float(exposure)
        self.twoview.rng_skip(3 * n)

    def Initialize(self, raw_u8, undistorter, exposure: float = 1.0, keys=None) -> bool:
        """One frame.  keys: the frame's mvKeys as a host (n, 2) array; without them they come from Frame::Extract's
        path on the device (makeMapsImage + extract_image)."""
        self.image.set_u8(undistorter, raw_u8)
        if keys is None:
            if self.extractor is None:
                raise ValueError("no extractor pattern was given: Initialize needs the frame's keys")
            self.selector.makeMapsImage(self.image, self.n_frames, self.density, want_map=False)
            n = self.extractor.extract_image(self.selector, self.image)
        else:
            keys = np.ascontiguousarray(keys, np.float32).reshape(-1, 2)
            n = len(keys)
        self.n_frames += 1
        entry_first, entry_fails = self.has_first, self.NumFails
        nmatches = mean = res = fit = None
        while True:
            d = decide(entry_first, entry_fails, n, self.n_first, nmatches, mean, fit)
            if d.action == NEED_TRACK:
                nmatches = self.flow.track_image(self.image, MAX_L1_ERROR)
            elif d.action == NEED_MEAN_FLOW:
                mean = self.flow.mean_flow_device()
            elif d.action == NEED_FIT:
                res = self.twoview.fit_flow_drawn(self.flow, self.n_sets)
                fit = (res.ok != 0, res.n_triangulated)
            else:
                break
        self.has_first, self.NumFails = d.has_first, d.num_fails
        if d.action == FIRST:
            self._take_first(keys, n, exposure)
        if res is not None:
            self.result = res
        if d.action == SUCCESS:                                      # :139-161
            self.refiner.set_second_image(self.image, exposure)
            self.refiner.set_points_twoview(self.flow, self.twoview)
            self.pose, _, self.good, it, snapped = self.refiner.Refine(pose_of(res))
            self.refine_stats = (it, snapped)
        self.history.append(dict(action=d.action, reset_at_entry=d.reset_at_entry, nFeatures=n, nmatches=d.nmatches,
                                 mean_flow=None if mean is None else float(mean),
                                 why=None if res is None else int(res.why), NumFails=self.NumFails,
                                 rng_state=self.twoview.rng_state()))
        return d.action == SUCCESS

    def init_window(self, ba):
        """System::InitFromInitializer up to AddKeyframe(secondFrame): the identity first frame, its image, the point
        loop.  Returns (why, handles, the firstToNew pose); the caller's next makeIDX commits the points."""
        from .ba import make_frame
        if self.pose is None:
            raise RuntimeError("Initialize has not succeeded yet")
        frame = ba.insertFrame(make_frame(IDENTITY, exposure=self.first_exposure, fid=0))
        ba.set_frame_image_from(frame, self.first_image)
        why, handles = self.refiner.seed_window(ba, frame)
        return why, handles, self.pose
