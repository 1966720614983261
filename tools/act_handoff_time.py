"""Times the hand-off around activatePointsMT on the keyframe path, through the host against on the device
(hs_tracer_activate_ba), one JSON line per size: python tools/act_handoff_time.py [--out FILE] [--kernel-stats CSV]

Sizes: 8 KF x 250 points per KF with 3000 immature points at 640x480, and the same at the KITTI size (1232x368).
Per keyframe the wall time from "newest frame inserted, residuals to it added" to "makeIDX done, tracer compacted,
both synchronised":
  host    hs_tracer_activate fed host arrays (formed beforehand, outside the timed region: the host path at its
          best), hs_tracer_get_points, hs_ba_insert_points, hs_ba_insert_residuals, hs_tracer_compact, makeIDX
  device  one hs_tracer_activate_ba call (compact = 1), makeIDX
The two paths alternate in one process; the (BA window, tracer) pair of every keyframe is rebuilt outside the timed
region; the figure of a repeat is the median of ROUNDS keyframes after WARMUP; REPEATS repeats give the spread
(max - min of the medians).  It also counts each path's structural commits inside the timed region (one
hs_k_win_gather launch each; hs_debug_commit_count) and checks that both paths end with the same window and tracer
sizes.  The activation call commits the pending edits before it reads the window ("commit_first": the simplest
correct form; the commit is not split into a frames half and a points half).

--once PATH runs only ROUNDS keyframes of one path ("host" / "device") at the first size, for a profiler run:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o act -- python tools/act_handoff_time.py --once device
--kernel-stats CSV adds the average us per launch of the new kernels from that run's *_kernel_stats.csv.
Not a test and no pass bar: a measurement."""
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "h-slam_amd"))
from hslam_amd import _lib  # noqa: E402
from hslam_amd.ba import BAWindow, make_frame  # noqa: E402
from hslam_amd.scene import make_window_activation_scene  # noqa: E402
from hslam_amd.trace import ImmatureTracer  # noqa: E402

WINDOW, POINTS_PER_KF, IMMATURE = 8, 250, 3000
WARMUP, ROUNDS, REPEATS = 3, 20, 3
CMAD = 2.0
NEW_KERNELS = ("hs_k_act_form", "hs_k_act_stage", "hs_k_cmp_flags", "hs_k_cmp_scan", "hs_k_cmp_scatter",
               "hs_k_win_gather")


def build(bs, s):
    """AddKeyframe up to the activation: frames 0 .. n-2 committed with their points, the newest frame inserted and
    the residuals to it added (both uncommitted); the tracer with every immature point."""
    nF = bs.n_frames
    ba = BAWindow(camera=(bs.width, bs.height, bs.n_levels, bs.K), capacity=2 * bs.n_points + IMMATURE)
    for f in range(nF - 1):
        ba.insertFrame(make_frame(bs.frames_eval[f], bs.frames_state[f], bs.frames_state_zero[f],
                                  bs.frames_exposure[f], bs.frames_energyTH[f], bs.frames_id[f]),
                       image=bs.pyramids[f][0])
    sel = np.nonzero(bs.pt_host < nF - 1)[0]
    hd = ba.insertPoints(bs.pt_host[sel], bs.pt_u[sel], bs.pt_v[sel], bs.pt_idepth[sel], bs.pt_idepth_zero[sel],
                         bs.pt_color[sel], bs.pt_weights[sel])
    handle = -np.ones(bs.n_points, np.int64)
    handle[sel] = hd
    r = (bs.res_target < nF - 1) & (handle[bs.res_point] >= 0)
    ba.insertResiduals(handle[bs.res_point[r]], bs.res_target[r])
    ba.makeIDX()
    ba.insertFrame(make_frame(bs.frames_eval[nF - 1], bs.frames_state[nF - 1], bs.frames_state_zero[nF - 1],
                              bs.frames_exposure[nF - 1], bs.frames_energyTH[nF - 1], bs.frames_id[nF - 1]),
                   image=bs.pyramids[nF - 1][0])
    ba.addResidualsToNewest()
    tr = ImmatureTracer(s.width, s.height, len(s.imm_u))
    for f in range(nF):
        tr.set_host_image(int(s.slots[f]), s.imgs[f])
    tr.add_points(s.slots[s.imm_frame], s.imm_u, s.imm_v)
    tr.set_state(s.imm_idepth_min, s.imm_idepth_max, s.imm_quality, s.imm_status, s.imm_interval)
    tr.set_types(s.imm_type)
    ba.synchronize()
    tr.points()  # the tracer's stream is idle
    return ba, tr


def commits(ba):
    return _lib.load().hs_debug_commit_count(ba.h)


def keyframe_device(bs, s, ba, tr):
    c0, t0 = commits(ba), time.perf_counter()
    tr.activate_into(ba, s.slots, s.flagged, CMAD, order=s.order, compact=True)
    ba.makeIDX()
    ba.synchronize()
    tr._count()
    return time.perf_counter() - t0, commits(ba) - c0


def keyframe_host(bs, s, ba, tr, i):
    nF = bs.n_frames
    c0, t0 = commits(ba), time.perf_counter()
    r = tr.activatePointsMT(i["K4"], i["frames"], i["pairs"], i["act_frame"], i["act_u"], i["act_v"], i["act_idepth"],
                            len(i["act_u"]), CMAD, s.order)
    a = r["activated"]
    pts = tr.points()
    hd = ba.insertPoints(s.imm_frame[a], s.imm_u[a], s.imm_v[a], r["idepth"][a], r["idepth"][a], pts["color"][a],
                         pts["weights"][a])
    bits = (r["res_in"][a][:, None] >> np.arange(nF)[None, :]) & 1
    k, t = np.nonzero(bits)
    ba.insertResiduals(hd[k], t)
    tr.compact((r["action"] == 0).astype(np.uint8))
    ba.makeIDX()
    ba.synchronize()
    tr._count()
    return time.perf_counter() - t0, commits(ba) - c0


def formed_inputs(bs, s):
    ba, tr = build(bs, s)
    tr.activate_into(ba, s.slots, s.flagged, CMAD, order=s.order, compact=False)
    i = tr.act_inputs(ba)
    ba.close()
    tr.close()
    return i


def one_repeat(bs, s, inputs, paths=("host", "device")):
    times = {m: [] for m in paths}
    ncommit = {m: set() for m in paths}
    sizes = {}
    for k in range(WARMUP + ROUNDS):
        for m in paths:
            ba, tr = build(bs, s)
            dt, nc = keyframe_device(bs, s, ba, tr) if m == "device" else keyframe_host(bs, s, ba, tr, inputs)
            if k >= WARMUP:
                times[m].append(dt)
                ncommit[m].add(nc)
            sizes[m] = (ba.n_points, ba.n_res, tr.n)
            ba.close()
            tr.close()
    return {m: float(np.median(t)) * 1e6 for m, t in times.items()}, ncommit, sizes


def measure(kitti):
    bs, s = make_window_activation_scene(n_active=WINDOW * POINTS_PER_KF, n_immature=IMMATURE, n_frames=WINDOW,
                                         **(dict(width=1232, height=368, kitti=True) if kitti
                                            else dict(width=640, height=480)))
    inputs = formed_inputs(bs, s)
    med = {"host": [], "device": []}
    ncommit = {"host": set(), "device": set()}
    same, sizes = True, {}
    for _ in range(REPEATS):
        r, nc, sizes = one_repeat(bs, s, inputs)
        same = same and sizes["host"] == sizes["device"]
        for m in med:
            med[m].append(r[m])
            ncommit[m] |= nc[m]
    out = {"size": f"{bs.width}x{bs.height}", "window": WINDOW, "points_per_kf": POINTS_PER_KF, "immature": IMMATURE,
           "points_after": int(sizes["device"][0]), "immature_after": int(sizes["device"][2]),
           "keyframes_per_repeat": ROUNDS, "repeats": REPEATS, "same_sizes": same, "activation_reads": "commit_first"}
    for m in med:
        out[f"{m}_us_medians"] = [round(v, 1) for v in med[m]]
        out[f"{m}_us"] = round(float(np.median(med[m])), 1)
        out[f"{m}_spread_us"] = round(max(med[m]) - min(med[m]), 1)
        out[f"{m}_gather_launches_per_keyframe"] = sorted(ncommit[m])
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
        bs, s = make_window_activation_scene(n_active=WINDOW * POINTS_PER_KF, n_immature=IMMATURE, n_frames=WINDOW,
                                             width=640, height=480)
        inputs = formed_inputs(bs, s) if args[1] == "host" else None
        r, nc, sizes = one_repeat(bs, s, inputs, paths=(args[1],))
        print(json.dumps({"path": args[1], "us": r[args[1]], "gather_launches_per_keyframe": sorted(nc[args[1]])}))
        sys.exit(0)
    lines = [measure(kitti) for kitti in (False, True)]
    if "--kernel-stats" in args:
        ks = kernel_stats(args[args.index("--kernel-stats") + 1])
        for ln in lines[:1]:
            ln["kernel_us_per_launch"] = ks
    text = "\n".join(json.dumps(ln) for ln in lines)
    print(text)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(text + "\n")
