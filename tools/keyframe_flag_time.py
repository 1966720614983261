"""Times flagPointsForRemoval on the keyframe path, decided on the host against decided on the device
(hs_ba_flag_points_for_removal), one JSON line per sequence: python tools/keyframe_flag_time.py [--out FILE]

Sequences: the C4 scene at 8 KF x 250 points per KF (640x480) and its KITTI variant (1232x368).  Per keyframe the wall
time from the end of the optimize tail to the end of removeFrame, closed by a synchronise: toRemove, removeOutliers,
the decisions, marginalizePointsF, the removals and marginalizeFrame.
  host    KeyframeBA(decisions="host"): the lastResiduals bookkeeping and the rule in numpy from three read-backs
          (structure, residual states, point state), then hs_ba_marginalize_points + hs_ba_remove_points
  device  KeyframeBA(decisions="device"): one hs_ba_flag_points_for_removal call
Both drivers run in the same process over the same sequence, alternating keyframe by keyframe, 3 warm-up keyframes and
then ROUNDS timed ones each; the figure of a repeat is the median.  REPEATS repeats (fresh drivers) give the spread
(max - min of the medians).  It also checks that both drivers marginalized and dropped the same points at every
keyframe.  Not a test and no pass bar: a measurement."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "h-slam_amd"))
from hslam_amd.keyframe import KeyframeBA, make_ba_sequence  # noqa: E402

WINDOW, POINTS_PER_KF = 8, 250
WARMUP, ROUNDS, REPEATS = 3, 20, 3


def one_repeat(seq):
    drv = {m: KeyframeBA(seq, window=WINDOW, decisions=m) for m in ("host", "device")}
    times = {m: [] for m in drv}
    mark = {}

    def check(d, phase):
        if phase == "tail":
            d.ba.synchronize()
            mark["t0"] = time.perf_counter()
        elif phase == "frame_marginalized":
            d.ba.synchronize()
            mark["dt"] = time.perf_counter() - mark["t0"]

    for d in drv.values():
        d.bootstrap()
    same = True
    for i, k in enumerate(range(WINDOW - 1, WINDOW - 1 + WARMUP + ROUNDS)):
        sets = {}
        for m, d in drv.items():
            d.add_keyframe(k, check=check)
            if i >= WARMUP:
                times[m].append(mark["dt"])
            sets[m] = (sorted(map(int, d.marg_handles)), sorted(map(int, d.drop_handles)))
        same = same and sets["host"] == sets["device"]
    n_points = drv["host"].history[-1]["n_points"]
    for d in drv.values():
        d.ba.close()
    return {m: float(np.median(t)) * 1e6 for m, t in times.items()}, same, n_points


def measure(kitti):
    seq = make_ba_sequence(n_kf=WINDOW - 1 + WARMUP + ROUNDS, points_per_kf=POINTS_PER_KF, kitti=kitti,
                           **(dict(width=1232, height=368) if kitti else {}))
    med = {"host": [], "device": []}
    same, n_points = True, 0
    for _ in range(REPEATS):
        r, s, n_points = one_repeat(seq)
        same = same and s
        for m in med:
            med[m].append(r[m])
    out = {"size": f"{seq.width}x{seq.height}", "window": WINDOW, "points_per_kf": POINTS_PER_KF,
           "points_in_window": int(n_points), "keyframes_per_repeat": ROUNDS, "repeats": REPEATS, "same_decisions": same}
    for m in med:
        out[f"{m}_us_medians"] = [round(v, 1) for v in med[m]]
        out[f"{m}_us"] = round(float(np.median(med[m])), 1)
        out[f"{m}_spread_us"] = round(max(med[m]) - min(med[m]), 1)
    return out


if __name__ == "__main__":
    lines = [json.dumps(measure(kitti)) for kitti in (False, True)]
    print("\n".join(lines))
    if len(sys.argv) > 2 and sys.argv[1] == "--out":
        with open(sys.argv[2], "w") as fh:
            fh.write("\n".join(lines) + "\n")
