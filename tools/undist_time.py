"""Times the undistortion of raw u8 frames (include/hs_undist.h) at the two shipped calibrations' sizes and prints one
JSON line: python tools/undist_time.py [--out FILE]

Per size: the kernel's device time (one event pair over 200 back-to-back launches after 20 warm-up launches, three
repeats), its algorithmic bytes (map 8 B + fImg 4 B per output pixel, raw 1 B per input pixel, + 4 B per input pixel
of vignette in the photometric configuration) and the rate they give; and the host-clock time of
CoarseTracker.setNewFrameU8 against setNewFrameRaw on the same frame, interleaved (both end in a stream
synchronise).  Not a test and no pass bar: a measurement."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "h-slam_amd"))
from hslam_amd.track import CoarseTracker  # noqa: E402
from hslam_amd.undistort import Undistorter, make_calib  # noqa: E402

EUROC_DIST = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
SIZES = {
    "752x480->640x480": make_calib("RadTan", 752, 480, 640, 480, (458.654, 457.296, 367.215, 248.375), EUROC_DIST,
                                   "useK", (0.6, 0.9, 0.5, 0.5)),
    "1241x376->1232x368": make_calib("Pinhole", 1241, 376, 1232, 368, (718.856, 718.856, 607.1928, 185.2157), (0.0,),
                                     "crop"),
}
CALLS = 100


def measure(calib):
    rng = np.random.default_rng(1)
    u = Undistorter(calib)
    n_in, n_out = u.w_in * u.h_in, u.w_out * u.h_out
    raw = rng.integers(0, 256, size=(u.h_in, u.w_in), dtype=np.uint8)
    out = {}
    for name, G, vig in (("plain", None, None),
                         ("photometric", ((np.arange(256) / 255.0) ** 0.8 * 200 + 3).astype(np.float32),
                          rng.integers(20000, 65536, size=raw.shape, dtype=np.uint16))):
        u.set_photometric(G, vig)
        us = [u.time_kernel(raw, 20, 200) * 1e3 for _ in range(3)]
        nbytes = n_out * 12 + n_in + (4 * n_in if vig is not None else 0)
        out[name] = {"kernel_us": [round(x, 2) for x in us], "bytes": nbytes,
                     "GB_per_s": round(nbytes / (min(us) * 1e-6) / 1e9, 1)}
    # the chained call against the float path on the same frame (photometric tables set), interleaved
    fimg, _ = u.undistort(raw, img8=False)
    k = u.K
    t = CoarseTracker(u.w_out, u.h_out, k, 4)
    for _ in range(5):
        t.setNewFrameU8(u, raw, 1.0)
        t.setNewFrameRaw(fimg, 1.0)
    tu, tr = [], []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        t.setNewFrameU8(u, raw, 1.0)
        t1 = time.perf_counter()
        t.setNewFrameRaw(fimg, 1.0)
        t2 = time.perf_counter()
        tu.append(t1 - t0)
        tr.append(t2 - t1)
    q = lambda a: [round(float(np.percentile(a, p)) * 1e6, 1) for p in (10, 50, 90)]  # noqa: E731
    out["setNewFrameU8_us_p10_p50_p90"] = q(tu)
    out["setNewFrameRaw_us_p10_p50_p90"] = q(tr)
    out["calls"] = CALLS
    t.close()
    u.close()
    return out


if __name__ == "__main__":
    line = json.dumps({k: measure(c) for k, c in SIZES.items()})
    print(line)
    if len(sys.argv) > 2 and sys.argv[1] == "--out":
        with open(sys.argv[2], "w") as f:
            f.write(line + "\n")
