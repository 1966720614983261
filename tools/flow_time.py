"""Times the initializer's keypoint tracking (include/hs_flow.h) at the two shipped calibrations' sizes, one JSON line
per size: python tools/flow_time.py [--out FILE]

Per size, the first frame's keys come from the selector -> extractor chain at density 2000 (hs_flow_set_first_extracted)
and the tracked frame is the same scene moved by (2.5, -1.25) px.  After 5 warm-up rounds and over 40 rounds that
alternate the two paths:
  extracted  hs_flow_track_extracted: cvImgL read where the extractor left it on the device
  host       hs_flow_track: cvImgL uploaded from the host
Both contexts are set back to the first frame before every round (outside the timed part), so every round tracks the
same points over the same motion.  Recorded: the device time of a track's kernels (pyramid, derivative, tracker) from
hs_flow_last_stats and the host-clock time of each call as p10 / median / p90 in microseconds, the keys, the good
points and the iterations run.  It also checks that both paths gave the same result.  Not a test and no pass bar: a
measurement."""
import json
import os
import sys
import time

import numpy as np
from scipy import ndimage

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "h-slam_amd"))
from hslam_amd.extract import FeatureExtractor  # noqa: E402
from hslam_amd.flow import KeypointFlow  # noqa: E402
from hslam_amd.scene import make_select_frames  # noqa: E402
from hslam_amd.select import PixelSelector  # noqa: E402

SIZES = ((640, 480), (1232, 368))
DENSITY = 2000
WARMUP, ROUNDS = 5, 40
CAPACITY = 8000
MAX_L1_ERROR = 7
SHIFT = (2.5, -1.25)


def measure(w, h):
    f0 = make_select_frames(1, width=w, height=h, contrast_ramp=True)[0]
    f1 = np.clip(ndimage.shift(f0, (SHIFT[1], SHIFT[0]), order=3, mode="nearest"), 0, 255)
    img0, img1 = np.rint(f0).astype(np.uint8), np.rint(f1).astype(np.uint8)
    pattern = np.random.default_rng(7).integers(-13, 14, size=(256, 2, 2), dtype=np.int8)
    sel = PixelSelector(w, h)
    ex0, ex1 = FeatureExtractor(w, h, CAPACITY, pattern), FeatureExtractor(w, h, CAPACITY, pattern)
    sel.makeMapsRaw(f0, 0, DENSITY, want_map=False)
    n_keys = ex0.extract_selected(sel, img0)           # the first frame: keys and cvImgL
    ex1.extract(np.zeros((h, w), np.float32), img1)    # the tracked frame: only its cvImgL is used
    a, b = KeypointFlow(w, h, CAPACITY), KeypointFlow(w, h, CAPACITY)
    keys = ex0.get()["xy"]

    t_ext, t_host, dev_ext, dev_host = [], [], [], []
    n_good = iters = 0
    for i in range(WARMUP + ROUNDS):
        a.set_first_extracted(ex0)
        b.set_first(img0, keys)
        t0 = time.perf_counter()
        na = a.track_extracted(ex1, MAX_L1_ERROR)
        t1 = time.perf_counter()
        nb = b.track(img1, MAX_L1_ERROR)
        t2 = time.perf_counter()
        assert na == nb, (na, nb)
        if i >= WARMUP:
            t_ext.append(t1 - t0)
            t_host.append(t2 - t1)
            dev_ext.append(a.last_stats()[0])
            dev_host.append(b.last_stats()[0])
            n_good, iters = na, a.last_stats()[1]
    ga, gb = a.get(), b.get()
    same = all(np.array_equal(ga[k], gb[k], equal_nan=True) for k in ga)
    flow = (ga["xy"] - ga["prev_xy"])[ga["good"] != 0]
    q = lambda v, s: [round(float(np.percentile(v, p)) * s, 1) for p in (10, 50, 90)]  # noqa: E731
    out = {"size": f"{w}x{h}", "density": DENSITY, "keys": n_keys, "good": n_good, "iterations": iters,
           "levels": a.last_stats()[2], "rounds": ROUNDS,
           "median_flow_px": [round(float(v), 3) for v in np.median(flow, axis=0)] if len(flow) else None,
           "track_extracted_kernels_us_p10_p50_p90": q(dev_ext, 1e3),
           "track_extracted_call_us_p10_p50_p90": q(t_ext, 1e6),
           "track_host_kernels_us_p10_p50_p90": q(dev_host, 1e3),
           "track_host_call_us_p10_p50_p90": q(t_host, 1e6),
           "same_result": bool(same)}
    for o in (a, b, ex0, ex1):
        o.close()
    return out


if __name__ == "__main__":
    lines = [json.dumps(measure(w, h)) for w, h in SIZES]
    print("\n".join(lines))
    if len(sys.argv) > 2 and sys.argv[1] == "--out":
        with open(sys.argv[2], "w") as fh:
            fh.write("\n".join(lines) + "\n")
