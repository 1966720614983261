"""Times one candidate second frame of the initializer from "tracked" to "the refiner holds its points", one JSON line
per size: python tools/initializer_time.py [--out FILE]

Per size (640x480 with 1773 keys, 1232x368 with 1385, 200 sets: the shapes of tools/twoview_time.py) the keys are
tracked by a KeypointFlow once; then, after one warm-up, over 3 repeats and from the same generator state:
  device   hs_flow_mean_flow_device + hs_twoview_fit_flow_drawn + hs_refiner_set_points_twoview: the host-clock time of
           each call, and the device time of the two draw kernels (hs_twoview_last_draw_stats) and of the fit's kernels
  parent   the same span through the entries that existed before: hs_flow_mean_flow (three key-sized read-backs and a
           host loop), hs_flow_get of the status, the draw of tests/initializer_ref.py on the host, hs_twoview_fit_flow
           with the uploaded sets, hs_refiner_set_points_twoview
Every number is the median of the 3 repeats with (min, max) as its spread.  The parent's draw is the Python model, the
only host draw over this generator the repository has: its time says what this repository's caller paid, not what a C++
caller with cv::RNG would.  Both paths must return the same record but the generator's state words (checked).  Not a
test and no pass bar: a measurement."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "h-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from initializer_ref import CvRng, draw_sets_cv  # noqa: E402
from hslam_amd.flow import KeypointFlow  # noqa: E402
from hslam_amd.refine import DirectRefinement  # noqa: E402
from hslam_amd.scene import make_refine_scene  # noqa: E402
from hslam_amd.twoview import TwoViewFit  # noqa: E402

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
    tv, tv_parent = TwoViewFit(n, s.K4), TwoViewFit(n, s.K4)
    r = DirectRefinement.bare(w, h, s.K4)
    r.set_frames(s.img1, s.img2, s.expo1, s.expo2)
    new = {k: [] for k in ("mean_flow_device", "fit_flow_drawn", "set_points_twoview", "span")}
    old = {k: [] for k in ("mean_flow", "flow_get_status", "model_draw", "fit_flow", "set_points_twoview", "span")}
    kern, draw_kern = [], []
    res = res_p = None
    same = True
    for i in range(1 + REPEATS):
        tv.rng_seed(0)
        t0 = time.perf_counter()
        mean = fl.mean_flow_device()
        t1 = time.perf_counter()
        res = tv.fit_flow_drawn(fl, N_SETS)
        t2 = time.perf_counter()
        if res.ok:
            r.set_points_twoview(fl, tv)
        t3 = time.perf_counter()
        rng = CvRng(0)
        p0 = time.perf_counter()
        mean_p = fl.mean_flow()
        p1 = time.perf_counter()
        good = fl.get()["good"]                                      # Python's get reads every array: timed below alone
        st = np.zeros(n, np.uint8)
        q0 = time.perf_counter()
        fl.lib.hs_flow_get(fl.h, None, None, None, None, None, None, st.ctypes.data)
        q1 = time.perf_counter()
        sets = draw_sets_cv(good, N_SETS, rng)
        q2 = time.perf_counter()
        res_p = tv_parent.fit_flow(fl, sets)
        q3 = time.perf_counter()
        if res_p.ok:
            r.set_points_twoview(fl, tv_parent)
        q4 = time.perf_counter()
        a, b = bytearray(bytes(res)), bytearray(bytes(res_p))
        a[104:112] = bytes(8)
        same = same and a == b and np.float32(mean).tobytes() == np.float32(mean_p).tobytes() \
            and tv.rng_state() == rng.state
        if i:
            for k, v in zip(new, (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
                new[k].append(v)
            parts = (p1 - p0, q1 - q0, q2 - q1, q3 - q2, q4 - q3)
            for k, v in zip(old, parts + (sum(parts),)):
                old[k].append(v)
            kern.append(tv.last_stats())
            draw_kern.append(tv.last_draw_stats())
    out = {"size": f"{w}x{h}", "keys": n, "good": n_good, "sets": N_SETS, "repeats": REPEATS, "ok": int(res.ok),
           "why": int(res.why), "n_triangulated": int(res.n_triangulated), "mean_flow": float(mean),
           "same_record_mean_and_state_as_parent_path": bool(same),
           "device_us_med_min_max": {k: stat(v) for k, v in new.items()},
           "parent_us_med_min_max": {k: stat(v) for k, v in old.items()},
           "draw_kernels_us_med_min_max": {k: stat([x[k] for x in draw_kern], 1e3) for k in draw_kern[0]},
           "fit_kernels_total_us_med_min_max": stat([sum(x.values()) for x in kern], 1e3)}
    for o in (r, tv, tv_parent, fl):
        o.close()
    return out


if __name__ == "__main__":
    lines = [json.dumps(measure(*c)) for c in CASES]
    print("\n".join(lines))
    if len(sys.argv) > 2 and sys.argv[1] == "--out":
        with open(sys.argv[2], "w") as fh:
            fh.write("\n".join(lines) + "\n")
