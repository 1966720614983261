"""Times the keyframe path's removals with and without a point map (include/hs_map.h), one JSON line per sequence:
python tools/map_time.py [--repeats N] [--out FILE]

Sequences: the C4 scene at 8 KF x 250 points per KF (640x480) and its KITTI variant (1232x368).  Per keyframe, from the
end of the optimize tail to the end of removeFrame, closed by a synchronise (toRemove, removeOutliers, the decisions,
marginalizePointsF, the removals and marginalizeFrame), by three routes:
  1 no_map     KeyframeBA(decisions="device"): tools/keyframe_flag_time.py's device route
  2 map        the same with a PointMap attached: the leaving points become records on the device
  3 readback   no map, but with the hs_ba_get_point_state + hs_ba_get_structure read-backs a caller needs before the
               flag call to keep the same data on the host
Two figures per route: wall (tail hook to frame_marginalized hook, as keyframe_flag_time.py measures it) and lib, the
time inside library calls only (the driver's "post" phase, plus the two read-backs on route 3).  The three drivers run in
the same process over the same sequence, alternating keyframe by keyframe, WARMUP warm-up keyframes and then ROUNDS
timed ones each; the figure of a repeat is the median, the repeats (fresh drivers) give the spread (max - min of the
medians).  It also checks that the three drivers removed the same points, and times one refresh_cloud call per window
frame at the end of a repeat.  Not a test and no pass bar: a measurement."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "h-slam_amd"))
from hslam_amd.keyframe import KeyframeBA, make_ba_sequence  # noqa: E402
from hslam_amd.map import PointMap  # noqa: E402

WINDOW, POINTS_PER_KF = 8, 250
WARMUP, ROUNDS = 3, 20
ROUTES = ("no_map", "map", "readback")


def one_repeat(seq):
    pmap = PointMap.create(POINTS_PER_KF * (WINDOW + WARMUP + ROUNDS + 2))
    drv = {r: KeyframeBA(seq, window=WINDOW, decisions="device", map=pmap if r == "map" else None) for r in ROUTES}
    wall = {r: [] for r in ROUTES}
    lib = {r: [] for r in ROUTES}
    mark = {}

    def hooks(route):
        def check(d, phase):
            if phase == "tail":
                d.ba.synchronize()
                mark["t0"] = time.perf_counter()
                mark["rb"] = 0.0
            elif phase == "marginalize" and route == "readback":
                t = time.perf_counter()
                mark["kept"] = (d.ba.point_state(), d.ba.structure())
                mark["rb"] = time.perf_counter() - t
            elif phase == "frame_marginalized":
                d.ba.synchronize()
                mark["dt"] = time.perf_counter() - mark["t0"]
        return check

    for d in drv.values():
        d.bootstrap()
    same = True
    for i, k in enumerate(range(WINDOW - 1, WINDOW - 1 + WARMUP + ROUNDS)):
        sets = {}
        for r, d in drv.items():
            info = d.add_keyframe(k, check=hooks(r))
            if i >= WARMUP:
                wall[r].append(mark["dt"])
                lib[r].append(info["phase_s"]["post"] + mark["rb"])
            sets[r] = (sorted(map(int, d.marg_handles)), sorted(map(int, d.drop_handles)))
        same = same and sets["no_map"] == sets["map"] == sets["readback"]
    # one refresh_cloud per window frame (the call: launch, count read-back, copies of the vertices and colours)
    d = drv["map"]
    cloud_us, cloud_pts = [], []
    for fid in d.frames:
        pmap.refresh_cloud(fid, d.ba)
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            c = pmap.refresh_cloud(fid, d.ba)
            ts.append(time.perf_counter() - t)
        cloud_us.append(float(np.median(ts)) * 1e6)
        cloud_pts.append(c["n"] // 8)
    n_points = drv["no_map"].history[-1]["n_points"]
    n_records = len(pmap)
    for d in drv.values():
        d.ba.close()
    pmap.close()
    med = lambda t: {r: float(np.median(v)) * 1e6 for r, v in t.items()}  # noqa: E731
    return med(wall), med(lib), same, n_points, n_records, float(np.median(cloud_us)), int(np.median(cloud_pts))


def measure(kitti, repeats):
    seq = make_ba_sequence(n_kf=WINDOW - 1 + WARMUP + ROUNDS, points_per_kf=POINTS_PER_KF, kitti=kitti,
                           **(dict(width=1232, height=368) if kitti else {}))
    wall = {r: [] for r in ROUTES}
    lib = {r: [] for r in ROUTES}
    same, n_points, n_records, cloud, cloud_pts = True, 0, 0, [], 0
    for _ in range(repeats):
        w, l, s, n_points, n_records, c, cloud_pts = one_repeat(seq)
        same = same and s
        cloud.append(c)
        for r in ROUTES:
            wall[r].append(w[r])
            lib[r].append(l[r])
    out = {"size": f"{seq.width}x{seq.height}", "window": WINDOW, "points_per_kf": POINTS_PER_KF,
           "points_in_window": int(n_points), "keyframes_per_repeat": ROUNDS, "repeats": repeats,
           "same_decisions": same, "records_per_repeat": int(n_records)}
    for name, t in (("wall", wall), ("lib", lib)):
        for r in ROUTES:
            out[f"{r}_{name}_us_medians"] = [round(v, 1) for v in t[r]]
            out[f"{r}_{name}_us"] = round(float(np.median(t[r])), 1)
            out[f"{r}_{name}_spread_us"] = round(max(t[r]) - min(t[r]), 1)
    out["refresh_cloud_call_us"] = round(float(np.median(cloud)), 1)
    out["refresh_cloud_kept_points"] = cloud_pts
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 3
    lines = [json.dumps(measure(kitti, repeats)) for kitti in (False, True)]
    print("\n".join(lines))
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write("\n".join(lines) + "\n")
