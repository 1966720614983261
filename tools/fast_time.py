"""Times the corner detector (hs_extractor_extract_fast, include/hs_extract.h) beside the map branch's extract on the
same frames, one JSON line per size: python tools/fast_time.py [--out FILE]

Sizes: 640x480 and 1232x368, one frame of make_select_frames each, the reference's detector settings (threshold 8,
3000 features, min_dist 5, tolerance 0.1).  Per size and repeat, after WARMUP calls, the median over ROUNDS calls of
  fast  extract_fast(cvImgL): the upload, the eight kernels, the 4-byte read of the count
  map   extract_selected(selector, cvImgL): the same with the keys scanned from the selector's map (density 2000)
as the wall time of the library call and as the device time between the call's two events (hs_extractor_last_stats).
The two alternate in one process; REPEATS repeats give the spread (max - min of the medians).

--once N [WxH] runs N fast extracts at that size (the first by default) and nothing else after the warm-up, for a
profiler run of its own, one per size:
  rocprofv3 --kernel-trace --hip-trace --stats --output-format csv -d DIR -o fast -- python tools/fast_time.py --once 40 640x480
--annotate FILE [--size WxH] [--kernel-stats CSV] [--api-stats CSV_A N_A CSV_B N_B] needs no device: it adds to FILE's
line of that size the average us per launch of every kernel of a fast extract from such a run's *_kernel_stats.csv, and the HIP calls
one extract makes, counted as the difference of two runs' *_hip_api_stats.csv over the difference of their N
(creation and warm-up cancel).  One wait and one read-back per extract show there as hipStreamSynchronize = 1 and
hipMemcpyAsync = 2 (cvImgL up, the count down).
Not a test and no pass bar: a measurement."""
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "h-slam_amd"))

SIZES = ((640, 480), (1232, 368))
DENSITY = 2000
WARMUP, ROUNDS, REPEATS = 5, 40, 3
CAPACITY = 8000
KERNELS = ("hs_k_fast_resp", "hs_k_fast_count", "hs_k_fast_write", "hs_k_fast_sort", "hs_k_fast_ssc",
           "hs_k_fast_final", "hs_k_ext_blur", "hs_k_ext_desc")
API = ("hipStreamSynchronize", "hipMemcpyAsync", "hipMemsetAsync", "hipLaunchKernel", "hipEventRecord")


def setup(w, h):
    from hslam_amd.extract import FeatureExtractor
    from hslam_amd.scene import make_select_frames
    f = make_select_frames(1, width=w, height=h, contrast_ramp=True)[0]
    img8 = np.rint(f).astype(np.uint8)
    pattern = np.random.default_rng(7).integers(-13, 14, size=(256, 2, 2), dtype=np.int8)
    return f, img8, FeatureExtractor(w, h, CAPACITY, pattern)


def measure(w, h):
    from hslam_amd.select import PixelSelector
    f, img8, ex = setup(w, h)
    sel = PixelSelector(w, h)
    sel.makeMapsRaw(f, 0, DENSITY, want_map=False)
    med = {k: [] for k in ("fast_us", "map_us", "fast_dev_us", "map_dev_us")}
    n_fast = n_map = 0
    for _ in range(REPEATS):
        t = {k: [] for k in med}
        for i in range(WARMUP + ROUNDS):
            t0 = time.perf_counter()
            n_fast = ex.extract_fast(img8)
            t1 = time.perf_counter()
            d_fast = ex.last_stats()
            t2 = time.perf_counter()
            n_map = ex.extract_selected(sel, img8)
            t3 = time.perf_counter()
            d_map = ex.last_stats()
            if i >= WARMUP:
                t["fast_us"].append((t1 - t0) * 1e6)
                t["map_us"].append((t3 - t2) * 1e6)
                t["fast_dev_us"].append(d_fast * 1e3)
                t["map_dev_us"].append(d_map * 1e3)
        for k in med:
            med[k].append(float(np.median(t[k])))
    ex.extract_fast(img8)
    info = ex.get_fast()
    out = {"size": f"{w}x{h}", "rounds": ROUNDS, "repeats": REPEATS, "corners": info["n_corners"],
           "ssc_width": info["width"], "fast_keys": n_fast, "map_keys": n_map, "ssc_form": "a workgroup per width"}
    for k, v in med.items():
        out[k] = round(float(np.median(v)), 1)
        out[k.replace("_us", "_spread_us")] = round(max(v) - min(v), 1)
    ex.close()
    return out


def once(n, size):
    _, img8, ex = setup(*size)
    for _ in range(WARMUP):
        ex.extract_fast(img8)
    keys = 0
    for _ in range(n):
        keys = ex.extract_fast(img8)
    ex.close()
    print(json.dumps({"once": n, "keys": keys}))


def rows(path):
    with open(path, newline="") as fh:
        return list(csv.DictReader(fh))


def kernel_stats(path):
    out = {}
    for row in rows(path):
        for k in KERNELS:
            if row["Name"].startswith(k + "(") or row["Name"] == k:
                out[k] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) * 1e-3, 2)}
    return out


def api_per_extract(path_a, n_a, path_b, n_b):
    calls = []
    for p in (path_a, path_b):
        calls.append({row["Name"]: int(row["Calls"]) for row in rows(p)})
    return {k: (calls[1].get(k, 0) - calls[0].get(k, 0)) / float(n_b - n_a) for k in API}


if __name__ == "__main__":
    args = sys.argv[1:]
    if len(args) >= 2 and args[0] == "--once":
        once(int(args[1]), tuple(map(int, args[2].split("x"))) if len(args) > 2 else SIZES[0])
        sys.exit(0)
    if len(args) >= 2 and args[0] == "--annotate":
        with open(args[1]) as fh:
            lines = [json.loads(ln) for ln in fh if ln.strip()]
        size = args[args.index("--size") + 1] if "--size" in args else "%dx%d" % SIZES[0]
        line = next(ln for ln in lines if ln["size"] == size)
        if "--kernel-stats" in args:
            line["kernel_us_per_launch"] = kernel_stats(args[args.index("--kernel-stats") + 1])
        if "--api-stats" in args:
            a = args[args.index("--api-stats") + 1:][:4]
            line["hip_calls_per_fast_extract"] = api_per_extract(a[0], int(a[1]), a[2], int(a[3]))
        with open(args[1], "w") as fh:
            fh.write("\n".join(json.dumps(ln) for ln in lines) + "\n")
        print("\n".join(json.dumps(ln) for ln in lines))
        sys.exit(0)
    lines = []
    for w, h in SIZES:
        lines.append(measure(w, h))
        print(f"measured {lines[-1]['size']}", file=sys.stderr, flush=True)
    text = "\n".join(json.dumps(ln) for ln in lines)
    print(text)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as fh:
            fh.write(text + "\n")
