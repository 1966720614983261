"""Times the keyframe driver's traced chain (KeyframeBA(points="traced")) with the trace hand-off on the device
(hs_tracer_trace_ba) against its host-fed twin (hs_tracer_trace on ready arrays), one JSON line per size:
  python tools/keyframe_chain_time.py [--out FILE] [--kernel-stats CSV]

Sizes: 640x480 and the KITTI size (1232x368); a window of 8 keyframes, every second frame a keyframe.
Protocol (tools/act_handoff_time.py's): both hand-offs alternate in one process, frame by frame, on two drivers over
one sequence, the first mover changing from one frame pair to the next (it touches the frame's data cold); a repeat
is WARMUP + ROUNDS keyframes (and as many traced non-keyframes) after the first window, its figure the median over the
ROUNDS; REPEATS repeats give the spread (max - min of the medians).  Per keyframe and per traced non-keyframe the
figure is the library wall time the driver records (its own numpy bookkeeping excluded); the host side's input arrays
are ready before its clock starts (what trace_inputs() returned at the same frame of an untimed device run made
beforehand: the chains are bit-identical).  Both sides wait for the trace's counts.  Beside it: the per-phase split of
a keyframe (frame, trace, setup, activate, optimize, tail, post, new_traces), optimize's time per GN iteration, and
whether the two chains ended with the same window and tracer sizes.

Quality (no bar): the median relative idepth error against render_depth_at's truth of the window's points that the
chain activated, read from the window as each later activation sees it (hs_tracer_get_act_inputs: host frame, u, v,
idepth of every window point, so each point has been through at least one optimize), beside the candidates driver's
points (true depth with 1 % noise, then optimized) on the same sequence.

--once PATH runs one repeat of one hand-off ("device" / "host") at the first size, for a profiler run:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o chain -- python tools/keyframe_chain_time.py --once device
--kernel-stats CSV adds hs_k_trc_form's (and hs_k_trace_on's) average us per launch from that run's *_kernel_stats.csv.
Not a test and no pass bar: a measurement."""
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "h-slam_amd"))
from hslam_amd.keyframe import KeyframeBA, make_ba_sequence  # noqa: E402
from hslam_amd.scene import render_depth_at, se3_from_data  # noqa: E402

WINDOW, POINTS_PER_KF = 8, 250
WARMUP, ROUNDS, REPEATS = 3, 20, 3
KEY_DENSITY = 1500.0
KERNELS = ("hs_k_trc_form", "hs_k_trace_on")
N_FRAMES = (WINDOW - 1) + 2 * (WARMUP + ROUNDS)


def make_sequence(kitti):
    return make_ba_sequence(n_kf=N_FRAMES, points_per_kf=POINTS_PER_KF, baseline=0.03, kitti=kitti,
                            **(dict(width=1232, height=368) if kitti else dict(width=640, height=480)))


def driver(seq, handoff, feed=None, record=False):
    return KeyframeBA(seq, window=WINDOW, decisions="device", points="traced", handoff=handoff, trace_feed=feed,
                      record_inputs=record, key_density=KEY_DENSITY, max_keys=4000)


def record_feed(seq):
    """The hs_trace_host arrays of every trace of the chain, from an untimed device run (the chains are bit-identical,
    so they are the arrays of the same commits in every later run)."""
    d = driver(seq, "device", record=True)
    run_all(seq, {"device": d})
    feed = d.trace_log
    d.close()
    return feed


def one_repeat(seq, feed, paths=("device", "host")):
    """Both chains frame by frame, each on its own driver."""
    drv = {m: driver(seq, m, feed if m == "host" else None) for m in paths}
    res = run_all(seq, drv)
    for d in drv.values():
        d.close()
    return res


def run_all(seq, drv):
    kf = {m: [] for m in drv}
    nkf = {m: [] for m in drv}
    phases = {m: [] for m in drv}
    for d in drv.values():
        d.bootstrap(WINDOW - 1)
    n_key = 0
    for k in range(WINDOW - 1, seq.n_frames):
        keyframe = (k - (WINDOW - 1)) % 2 == 1
        # who goes first alternates from one frame pair to the next: the first mover touches the frame's data cold
        order = list(drv.items())[::-1] if (k // 2) % 2 else list(drv.items())
        for m, d in order:
            if keyframe:
                info = d.add_keyframe(k)
                if n_key >= WARMUP:
                    kf[m].append(info["lib_s"])
                    phases[m].append(info["phase_s"])
            else:
                r = d.trace_frame(k)
                if n_key >= WARMUP:
                    nkf[m].append(r["lib_s"])
        n_key += keyframe
    out = {}
    for m, d in drv.items():
        ph = {p: round(float(np.median([x.get(p, 0.0) for x in phases[m]])) * 1e6, 1) for p in phases[m][0]}
        out[m] = dict(keyframe_us=float(np.median(kf[m])) * 1e6, non_keyframe_us=float(np.median(nkf[m])) * 1e6,
                      phases_us=ph, sizes=(d.ba.n_points, d.ba.n_res, d.tracer.n),
                      activated=[h["n_activated"] for h in d.history], keys=[h["n_keys"] for h in d.history],
                      gn_step_us=float(np.median([h["phase_s"]["optimize"] / max(1, h["iters"]) for h in d.history]))
                      * 1e6)
    return out


def truth_idepth(seq, k, u, v):
    R_w2c, t_w2c = se3_from_data(seq.poses[k])
    R_c2w = R_w2c.T
    C = -R_c2w @ t_w2c
    _, depth = render_depth_at(seq.planes, seq.K, R_c2w, C, np.stack([v, u], 1))
    return 1.0 / depth


def quality(seq):
    """Median relative idepth error of the window's activated (traced) points, and of the candidates driver's."""
    d = driver(seq, "device")
    seen = []
    inner = d.tracer.activate_into

    def wrapped(ba, *a, **k):
        r = inner(ba, *a, **k)
        i = d.tracer.act_inputs(ba)
        seen.append((list(d.frames), i))
        return r

    d.tracer.activate_into = wrapped
    d.bootstrap(WINDOW - 1)
    for k in range(WINDOW - 1, seq.n_frames):
        if (k - (WINDOW - 1)) % 2 == 1:
            d.add_keyframe(k)
        else:
            d.trace_frame(k)
    err_t, err_c = [], []
    for frames, i in seen[WARMUP:]:
        fr = np.asarray(frames)[i["act_frame"]]
        for k in np.unique(fr):
            s = fr == k
            u, v, idp = i["act_u"][s], i["act_v"][s], i["act_idepth"][s]
            c = seq.cand[k]
            planted = {(float(a), float(b)) for a, b in zip(c["u"], c["v"])}
            is_c = np.array([(float(a), float(b)) in planted for a, b in zip(u, v)], bool)
            e = np.abs(idp / truth_idepth(seq, k, u, v) - 1.0)
            err_t += e[~is_c & np.isfinite(e)].tolist()
            err_c += e[is_c & np.isfinite(e)].tolist()
    d.close()
    # the candidates driver on the same keyframes
    c = KeyframeBA(seq, window=WINDOW, decisions="device")
    c.bootstrap(WINDOW - 1)
    err_cd = []
    for k in range(WINDOW - 1, seq.n_frames):
        if (k - (WINDOW - 1)) % 2 == 1:
            c.add_keyframe(k)
    st, idp = c.ba.structure(), c.ba.points()["idepth"]
    for pos, hd in enumerate(st["handles"]):
        hk, ci = c.cand_of[int(hd)]
        err_cd.append(abs(idp[pos] / c.seq.cand[hk]["idepth_true"][ci] - 1.0))
    c.close()
    med = lambda x: round(float(np.median(x)), 5) if len(x) else None  # noqa: E731
    return dict(traced_points=len(err_t), traced_median_rel_idepth_err=med(err_t),
                traced_chain_candidates_median_rel_idepth_err=med(err_c),
                candidates_driver_points=len(err_cd), candidates_driver_median_rel_idepth_err=med(err_cd))


def measure(kitti):
    seq = make_sequence(kitti)
    med = {m: {"keyframe_us": [], "non_keyframe_us": [], "gn_step_us": []} for m in ("device", "host")}
    last, same = None, True
    feed = record_feed(seq)
    for _ in range(REPEATS):
        last = one_repeat(seq, feed)
        same = same and last["device"]["sizes"] == last["host"]["sizes"]
        for m in med:
            for q in med[m]:
                med[m][q].append(last[m][q])
    out = {"size": f"{seq.width}x{seq.height}", "window": WINDOW, "frames": seq.n_frames, "key_density": KEY_DENSITY,
           "keyframes_per_repeat": ROUNDS, "repeats": REPEATS, "same_sizes": same,
           "sizes_points_res_immature": [int(x) for x in last["device"]["sizes"]],
           "keys_per_keyframe_median": float(np.median(last["device"]["keys"])),
           "activated_per_keyframe_median": float(np.median(last["device"]["activated"]))}
    for m in med:
        for q, v in med[m].items():
            out[f"{m}_{q}_medians"] = [round(x, 1) for x in v]
            out[f"{m}_{q}"] = round(float(np.median(v)), 1)
            out[f"{m}_{q}_spread"] = round(max(v) - min(v), 1)
        out[f"{m}_phases_us"] = last[m]["phases_us"]
    out["quality"] = quality(seq)
    return out


def kernel_stats(path):
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            for k in KERNELS:
                if row["Name"].startswith(k + "("):
                    out[k] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) * 1e-3, 2)}
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) >= 2 and args[0] == "--once":
        seq0 = make_sequence(False)
        r = one_repeat(seq0, record_feed(seq0) if args[1] == "host" else None, paths=(args[1],))[args[1]]
        print(json.dumps({"path": args[1], "keyframe_us": r["keyframe_us"], "non_keyframe_us": r["non_keyframe_us"]}))
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
