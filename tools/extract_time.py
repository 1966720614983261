"""Times the keyframe hand-off selector -> extractor -> tracer (include/hs_extract.h) at the two shipped calibrations'
sizes, one JSON line per size: python tools/extract_time.py [--out FILE]

Per size, on one frame with a selector map at density 2000, after 5 warm-up rounds and over 40 rounds that alternate
the two paths (each ends in a synchronise of the tracer's stream):
  new     makeMapsRaw without map_out -> extract_selected -> add_keys: the map and the keys stay on the device; this
          path also uploads cvImgL and computes the blur, the angles and the descriptors
  parent  makeMapsRaw with map_out -> numpy raster scan of the interior -> add_points: what the library offered for
          the same immature points before the extractor existed (no descriptors)
and the device time of the extract's kernels from hs_extractor_last_stats.  Times are p10 / median / p90 in
microseconds; `spread_us` is the larger p90 - p10 of the two paths.  It also checks that both paths left the tracer
with the same points.  Not a test and no pass bar: a measurement."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "h-slam_amd"))
from hslam_amd.extract import BORDER, FeatureExtractor  # noqa: E402
from hslam_amd.scene import make_select_frames  # noqa: E402
from hslam_amd.select import PixelSelector  # noqa: E402
from hslam_amd.trace import ImmatureTracer  # noqa: E402

SIZES = ((640, 480), (1232, 368))
DENSITY = 2000
WARMUP, ROUNDS = 5, 40
CAPACITY = 8000


def wait(tr):
    """Synchronises the tracer's stream: a read-back that copies nothing."""
    n = C.c_int()
    rc = tr.lib.hs_tracer_get_points(tr.h, C.byref(n), *([None] * 10))
    assert rc == 0
    return n.value


def clear(tr):
    assert tr.lib.hs_tracer_clear(tr.h) == 0
    tr.n = 0


def measure(w, h):
    f = make_select_frames(1, width=w, height=h, contrast_ramp=True)[0]
    img8 = np.rint(f).astype(np.uint8)
    dir0 = np.zeros((h, w, 3), np.float32)
    dir0[..., 0] = f
    pattern = np.random.default_rng(7).integers(-13, 14, size=(256, 2, 2), dtype=np.int8)
    sel_new, sel_par = PixelSelector(w, h), PixelSelector(w, h)
    ex = FeatureExtractor(w, h, CAPACITY, pattern)
    tr_new, tr_par = ImmatureTracer(w, h, CAPACITY), ImmatureTracer(w, h, CAPACITY)
    for t in (tr_new, tr_par):
        t.set_host_image(0, dir0)

    def new_path(i):
        clear(tr_new)
        sel_new.makeMapsRaw(f, i, DENSITY, want_map=False)
        ex.extract_selected(sel_new, img8)
        tr_new.add_keys(ex, 0)
        return wait(tr_new)

    def parent_path(i):
        clear(tr_par)
        m, _ = sel_par.makeMapsRaw(f, i, DENSITY)
        ys, xs = np.nonzero(m[BORDER:h - BORDER, BORDER:w - BORDER])
        tr_par.add_points(np.zeros(len(xs), np.int32), (xs + BORDER).astype(np.float32),
                          (ys + BORDER).astype(np.float32))
        return wait(tr_par)

    t_new, t_par, dev_ms, n_keys = [], [], [], 0
    for i in range(WARMUP + ROUNDS):
        t0 = time.perf_counter()
        na = new_path(i)
        t1 = time.perf_counter()
        nb = parent_path(i)
        t2 = time.perf_counter()
        assert na == nb, (na, nb)   # both selectors walk the same potential sequence
        if i >= WARMUP:
            t_new.append(t1 - t0)
            t_par.append(t2 - t1)
            dev_ms.append(ex.last_stats())
            n_keys = na
    pa, pb = tr_new.points(), tr_par.points()
    same = all(np.array_equal(pa[k], pb[k], equal_nan=True) for k in pa)
    q = lambda a, s: [round(float(np.percentile(a, p)) * s, 1) for p in (10, 50, 90)]  # noqa: E731
    qn, qp = q(t_new, 1e6), q(t_par, 1e6)
    out = {"size": f"{w}x{h}", "density": DENSITY, "keys": n_keys, "rounds": ROUNDS,
           "extract_kernels_us_p10_p50_p90": q(dev_ms, 1e3),
           "new_handoff_us_p10_p50_p90": qn, "parent_path_us_p10_p50_p90": qp,
           "spread_us": round(max(qn[2] - qn[0], qp[2] - qp[0]), 1), "same_points": bool(same)}
    for t in (tr_new, tr_par):
        t.close()
    ex.close()
    return out


if __name__ == "__main__":
    lines = [json.dumps(measure(w, h)) for w, h in SIZES]
    print("\n".join(lines))
    if len(sys.argv) > 2 and sys.argv[1] == "--out":
        with open(sys.argv[2], "w") as fh:
            fh.write("\n".join(lines) + "\n")
