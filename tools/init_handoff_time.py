"""Times one initialization hand-off, through the host against on the device (include/hs_init.h), one JSON line per
size: python tools/init_handoff_time.py [--out FILE] [--kernel-stats CSV]

Sizes: 2000 keys (85 % triangulated) at 640x480 and at the KITTI size (1232x368).  The wall time of one hand-off runs
from "second frame tracked, tri / z on the host" (both frames lie in device images, the keys in the flow context, the
first window frame is inserted with its image) to "window committed with the seeded points, both synchronised":
  host    hs_image_get of both frames, hs_refiner_set_frames, hs_refiner_set_points, hs_refiner_refine (its videpth
          write-back is the read-back), hs_tracer_set_host_image + hs_tracer_add_points at +0.5 + hs_tracer_get_points
          (the ImmaturePoint constructor), hs_ba_insert_points, hs_ba_set_last_residuals, makeIDX
  device  hs_refiner_set_first_image, hs_refiner_set_second_image, hs_refiner_set_points_flow, hs_refiner_refine (pose
          only), hs_refiner_seed_ba, makeIDX
Both run the same Refine (the LM loop's own time is in both figures and reported apart, "refine_ms").  The two paths
alternate in one process; every object of a hand-off is rebuilt outside the timed region; the figure of a repeat is the
median of ROUNDS hand-offs after WARMUP; REPEATS repeats give the spread (max - min of the medians).  It checks that
both paths end with the same number of window points.

--once PATH runs only ROUNDS hand-offs of one path ("host" / "device") at the first size, for a profiler run:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o init -- python tools/init_handoff_time.py --once device
--kernel-stats CSV adds the average us per launch of the new kernels from that run's *_kernel_stats.csv.
Not a test and no pass bar: a measurement."""
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "h-slam_amd"))
from hslam_amd.ba import BAWindow, make_frame  # noqa: E402
from hslam_amd.flow import KeypointFlow  # noqa: E402
from hslam_amd.image import DeviceImage  # noqa: E402
from hslam_amd.refine import DirectRefinement  # noqa: E402
from hslam_amd.scene import make_refine_scene  # noqa: E402
from hslam_amd.trace import ImmatureTracer  # noqa: E402

KEYS = 2000
WARMUP, ROUNDS, REPEATS = 3, 20, 3
NEW_KERNELS = ("hs_k_ref_points", "hs_k_init_seed", "hs_k_win_gather")
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def make_scene(kitti):
    if kitti:
        return make_refine_scene(KEYS, width=1232, height=368,
                                 K=np.array([[718.856, 0, 615.5], [0, 718.856, 183.5], [0, 0, 1.0]]))
    return make_refine_scene(KEYS)


def build(s, fimg, img8, xy):
    """Everything a hand-off starts from: the two frames in device images, the flow after one track, a refiner without
    frames or points, a tracer, and the window with its first frame."""
    ims = []
    for f in fimg:
        im = DeviceImage(s.width, s.height, 1)
        im.set_raw(f)
        ims.append(im)
    fl = KeypointFlow(s.width, s.height, len(xy))
    fl.set_first(img8[0], xy)
    fl.track(img8[1], 7)
    r = DirectRefinement.bare(s.width, s.height, s.K4)
    tr = ImmatureTracer(s.width, s.height, len(xy))
    ba = BAWindow(camera=(s.width, s.height, 1, s.K), capacity=len(xy))
    ba.insertFrame(make_frame(IDENTITY, fid=0))
    ba.set_frame_image_from(0, ims[0])
    ba.synchronize()
    for im in ims:
        im.get(0)  # the images' streams are idle
    return ims, fl, r, tr, ba


def handoff_device(s, ims, fl, r, tr, ba):
    t0 = time.perf_counter()
    r.set_first_image(ims[0], s.expo1)
    r.set_second_image(ims[1], s.expo2)
    r.set_points_flow(fl, s.tri, s.z)
    r.Refine(s.T_init)
    r.seed_window(ba, 0)
    ba.makeIDX()
    ba.synchronize()
    return time.perf_counter() - t0, r.last_ms()


def handoff_host(s, ims, fl, r, tr, ba, vid0):
    t0 = time.perf_counter()
    d1, d2 = ims[0].get(0)[0], ims[1].get(0)[0]
    r.set_frames(d1, d2, s.expo1, s.expo2)
    r.set_points(s.u, s.v, s.tri, s.z)
    _, vid, _, _, _ = r.Refine(s.T_init, videpth=vid0)
    ms = r.last_ms()
    x, y = s.u.astype(np.float32) + np.float32(0.5), s.v.astype(np.float32) + np.float32(0.5)
    cand = np.nonzero((vid > 0) & (x >= 2) & (y >= 2) & (x < s.width - 3) & (y < s.height - 3))[0]
    tr.set_host_image(0, d1)
    tr.add_points(np.zeros(len(cand), np.int32), x[cand], y[cand])
    p = tr.points()
    fin = np.isfinite(p["energyTH"])
    keep = cand[fin]
    hd = ba.insertPoints(np.zeros(len(keep), np.int32), x[keep], y[keep], vid[keep], vid[keep], p["color"][fin],
                         p["weights"][fin], has_prior=np.ones(len(keep), np.uint8))
    ba.setLastResiduals(hd, -np.ones((len(keep), 2), np.int32), np.zeros((len(keep), 2), np.uint8))
    ba.makeIDX()
    ba.synchronize()
    return time.perf_counter() - t0, ms


def one_repeat(s, paths=("host", "device")):
    fimg = [np.ascontiguousarray(s.img1[..., 0]), np.ascontiguousarray(s.img2[..., 0])]
    img8 = [np.clip(np.rint(f), 0, 255).astype(np.uint8) for f in fimg]
    xy = np.stack([s.u, s.v], 1).astype(np.float32)
    vid0 = np.where(s.tri == 1, (1.0 / s.z.astype(np.float64)).astype(np.float32), np.float32(-1)).astype(np.float32)
    times = {m: [] for m in paths}
    refine = {m: [] for m in paths}
    points = {}
    for k in range(WARMUP + ROUNDS):
        for m in paths:
            ims, fl, r, tr, ba = build(s, fimg, img8, xy)
            dt, ms = handoff_device(s, ims, fl, r, tr, ba) if m == "device" else handoff_host(s, ims, fl, r, tr, ba, vid0)
            if k >= WARMUP:
                times[m].append(dt)
                refine[m].append(ms)
            points[m] = ba.n_points
            for o in (r, tr, ba, fl, *ims):
                o.close()
    return ({m: float(np.median(t)) * 1e6 for m, t in times.items()},
            {m: float(np.median(t)) for m, t in refine.items()}, points)


def measure(kitti):
    s = make_scene(kitti)
    med = {"host": [], "device": []}
    ref = {"host": [], "device": []}
    same, points = True, {}
    for _ in range(REPEATS):
        r, ms, points = one_repeat(s)
        same = same and points["host"] == points["device"]
        for m in med:
            med[m].append(r[m])
            ref[m].append(ms[m])
    out = {"size": f"{s.width}x{s.height}", "keys": KEYS, "triangulated": int(s.tri.sum()),
           "points_seeded": int(points["device"]), "handoffs_per_repeat": ROUNDS, "repeats": REPEATS,
           "same_points": same}
    for m in med:
        out[f"{m}_us_medians"] = [round(v, 1) for v in med[m]]
        out[f"{m}_us"] = round(float(np.median(med[m])), 1)
        out[f"{m}_spread_us"] = round(max(med[m]) - min(med[m]), 1)
        out[f"{m}_refine_ms"] = round(float(np.median(ref[m])), 3)
    return out


def kernel_stats(path):
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            for k in NEW_KERNELS:
                if row["Name"].startswith(k + "("):
                    out[k] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) * 1e-3, 2)}
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) >= 2 and args[0] == "--once":
        r, ms, points = one_repeat(make_scene(False), paths=(args[1],))
        print(json.dumps({"path": args[1], "us": r[args[1]], "refine_ms": ms[args[1]], "points": points[args[1]]}))
        sys.exit(0)
    lines = []
    for kitti in (False, True):
        lines.append(measure(kitti))
        print(f"measured {lines[-1]['size']}", file=sys.stderr, flush=True)
    if "--kernel-stats" in args:
        ks = kernel_stats(args[args.index("--kernel-stats") + 1])
        for ln in lines[:1]:
            ln["kernel_us_per_launch"] = ks
    text = "\n".join(json.dumps(ln) for ln in lines)
    print(text)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(text + "\n")
