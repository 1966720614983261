"""Times the initializer's two-view fit (include/hs_twoview.h) and its hand-off into the refiner, one JSON line per
size: python tools/twoview_time.py [--out FILE]

Per size (640x480 with 1773 keys, 1232x368 with 1385: the key counts of profiles/flow_time.jsonl) the two frames are the
textured-plane world of hslam_amd.scene.make_refine_scene with a baseline that the tracker follows and the fit accepts;
the keys are tracked by a KeypointFlow, and 200 sets are drawn from the good ones.  After one warm-up, over 3 repeats:
  device   hs_twoview_fit_flow + hs_refiner_set_points_twoview: the host-clock time of the two calls, and the device time
           of each of the fit's kernels (hs_twoview_last_stats)
  today    the same hand-off through the entries that existed before: hs_flow_get, the caller's own fit (here the numpy
           model tests/twoview_ref.py, the only host fit this repository has), hs_refiner_set_points_flow
Every number is the median of the 3 repeats with (min, max) as its spread.  The numpy model is a model, not an optimized
host fit: its time says what a caller without a fit of its own would pay here, not what OpenCV would.  Not a test and no
pass bar: a measurement."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "h-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import twoview_ref as tr  # noqa: E402
from hslam_amd.flow import KeypointFlow  # noqa: E402
from hslam_amd.refine import DirectRefinement  # noqa: E402
from hslam_amd.scene import make_refine_scene  # noqa: E402
from hslam_amd.twoview import TwoViewFit, draw_sets  # noqa: E402

KITTI_K = np.array([[718.856, 0, 615.5], [0, 718.856, 183.5], [0, 0, 1.0]])
CASES = ((640, 480, 1773, None, 0.10), (1232, 368, 1385, KITTI_K, 0.05))
N_SETS, REPEATS = 200, 3
MAX_L1_ERROR = 7


def stat(v, scale=1e6):
    v = sorted(float(x) * scale for x in v)
    return [round(v[len(v) // 2], 1), round(v[0], 1), round(v[-1], 1)]


def measure(w, h, n, K, trans):
    s = make_refine_scene(n, width=w, height=h, K=K, tri_frac=0.6, trans=trans)
    img8 = lambda f: np.clip(np.rint(f), 0, 255).astype(np.uint8)  # noqa: E731
    xy = np.stack([s.u, s.v], 1).astype(np.float32)
    fl = KeypointFlow(w, h, n)
    fl.set_first(img8(s.img1[..., 0]), xy)
    n_good = fl.track(img8(s.img2[..., 0]), MAX_L1_ERROR)
    sets = draw_sets(N_SETS, fl.get()["good"], np.random.default_rng(0))
    tv = TwoViewFit(n, s.K4)
    r = DirectRefinement.bare(w, h, s.K4)
    r.set_frames(s.img1, s.img2, s.expo1, s.expo2)
    t_fit, t_set, t_get, t_model, t_setflow, kern = [], [], [], [], [], []
    res = model = None
    for i in range(1 + REPEATS):
        t0 = time.perf_counter()
        res = tv.fit_flow(fl, sets)
        t1 = time.perf_counter()
        if res.ok:
            r.set_points_twoview(fl, tv)
        t2 = time.perf_counter()
        g = fl.get()
        t3 = time.perf_counter()
        model = tr.fit(g["first_xy"], g["xy"], g["good"], sets, s.K4)
        t4 = time.perf_counter()
        if model["ok"]:
            r.set_points_flow(fl, model["triangulated"], model["p3d"][:, 2])
        t5 = time.perf_counter()
        if i:
            t_fit.append(t1 - t0)
            t_set.append(t2 - t1)
            t_get.append(t3 - t2)
            t_model.append(t4 - t3)
            t_setflow.append(t5 - t4)
            kern.append(tv.last_stats())
    out = {"size": f"{w}x{h}", "keys": n, "good": n_good, "sets": N_SETS, "repeats": REPEATS,
           "ok": int(res.ok), "why": int(res.why), "model": "F" if res.model == 1 else "H",
           "inliers": int(res.n_inliers), "n_triangulated": int(res.n_triangulated),
           "parallax_deg": round(float(res.parallax_deg), 3),
           "same_decision_as_model": bool((res.ok, res.model, res.best_h, res.best_f, res.best_rt)
                                          == (model["ok"], model["model"], model["best_h"], model["best_f"],
                                              model["best_rt"])),
           "jacobi": "one wave per (set, model)", "score_keys": "read through L2 (no LDS staging)",
           "fit_flow_call_us_med_min_max": stat(t_fit), "set_points_twoview_call_us_med_min_max": stat(t_set),
           "device_handoff_us_med_min_max": stat([a + b for a, b in zip(t_fit, t_set)]),
           "kernels_us_med_min_max": {k: stat([x[k] for x in kern], 1e3) for k in kern[0]},
           "kernels_total_us_med_min_max": stat([sum(x.values()) for x in kern], 1e3),
           "today_flow_get_us_med_min_max": stat(t_get), "today_numpy_model_fit_us_med_min_max": stat(t_model),
           "today_set_points_flow_us_med_min_max": stat(t_setflow),
           "today_handoff_us_med_min_max": stat([a + b + c for a, b, c in zip(t_get, t_model, t_setflow)])}
    for o in (r, tv, fl):
        o.close()
    return out


if __name__ == "__main__":
    lines = [json.dumps(measure(*c)) for c in CASES]
    print("\n".join(lines))
    if len(sys.argv) > 2 and sys.argv[1] == "--out":
        with open(sys.argv[2], "w") as fh:
            fh.write("\n".join(lines) + "\n")
