"""Times the device frame (include/hs_image.h) at the two shipped calibrations' sizes, one JSON line per size:
python tools/image_time.py [--out FILE]

Per size (640x480 with 4 levels, 1232x368 with 5), on one textured raw u8 frame, after 5 warm-up rounds and over 40
rounds that alternate the hand-off's two sides:
  build    device time of one frame's build: hs_image_set_u8's two kernels (hs_image_last_stats)
  handoff  one keyframe's image hand-off, from the raw u8 frame in host memory to tracker frame, tracer frame, tracer
           host slot, selector map, extractor result and BA window image all set, each path ending in a synchronise of
           the device:
             new     one hs_image_set_u8 and the six consumer entries
             parent  hs_tracker_set_frame_u8, hs_tracer_set_frame_u8, hs_undistorter_apply -> host fImgL ->
                     hs_selector_make_maps_raw, hs_dir_pyramid's level 0 on the host -> hs_tracer_set_host_image,
                     hs_extractor_extract_u8, hs_tracker_frame_to_ba: each leg as the library offered it before
Times are p10 / median / p90 in microseconds; `build_spread_us` is the build's p90 - p10, `handoff_spread_us` the
larger p90 - p10 of the two sides.  The tool also asserts that both paths leave the consumers bit-equal.  Not a test
and no pass bar: a measurement."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "h-slam_amd"))
from hslam_amd.ba import BAWindow  # noqa: E402
from hslam_amd.extract import FeatureExtractor  # noqa: E402
from hslam_amd.image import DeviceImage  # noqa: E402
from hslam_amd.pyr import dir_pyramid  # noqa: E402
from hslam_amd.scene import make_ba_scene, make_select_frames  # noqa: E402
from hslam_amd.select import PixelSelector  # noqa: E402
from hslam_amd.trace import ImmatureTracer  # noqa: E402
from hslam_amd.track import CoarseTracker  # noqa: E402
from hslam_amd.undistort import Undistorter, make_calib  # noqa: E402

EUROC_DIST = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)
CASES = (
    dict(calib=make_calib("RadTan", 752, 480, 640, 480, (458.654, 457.296, 367.215, 248.375), EUROC_DIST, "useK",
                          (0.6, 0.9, 0.5, 0.5)), levels=4, kitti=False),
    dict(calib=make_calib("Pinhole", 1241, 376, 1232, 368, (718.856, 718.856, 607.1928, 185.2157), (0.0,), "crop"),
         levels=5, kitti=True),
)
DENSITY = 2000
WARMUP, ROUNDS = 5, 40
CAPACITY = 8000
SLOT, FRAME = 2, 2


def hip():
    with open("/proc/self/maps") as maps:
        path = next(line.split()[-1] for line in maps if "libamdhip64" in line)
    lib = C.CDLL(path)
    lib.hipMemcpy.argtypes, lib.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    lib.hipDeviceSynchronize.argtypes, lib.hipDeviceSynchronize.restype = [], C.c_int
    return lib


class Consumers:
    def __init__(self, w, h, levels, scene, pattern):
        self.trk = CoarseTracker(w, h, scene.K[[0, 1, 0, 1], [0, 1, 2, 2]], levels)
        self.trc = ImmatureTracer(w, h, CAPACITY)
        self.sel = PixelSelector(w, h)
        self.ex = FeatureExtractor(w, h, CAPACITY, pattern)
        self.ba = BAWindow(scene)
        self.ba.linearizeAll(reset=True)    # the window is incremental and committed before the timed rounds

    def observe(self, lib, levels):
        """What the hand-off left: tracker texels, host-slot point colours, selector map, keys, BA energy."""
        assert lib.hipDeviceSynchronize() == 0
        out = []
        for l in range(levels):
            a = np.empty((self.trk.hl[l], self.trk.wl[l], 4), np.float32)
            assert lib.hipMemcpy(a.ctypes.data, self.trk.frame_texels(l), a.nbytes, 2) == 0
            out.append(a)
        g = self.ex.get(blurred=True)
        out += [g[k] for k in sorted(g)]
        xy = g["xy"][:500]
        self.trc.add_points(np.full(len(xy), SLOT, np.int32), xy[:, 0], xy[:, 1])
        eye = np.tile(np.eye(3, dtype=np.float32).ravel(), (SLOT + 1, 1))
        Kt = np.tile(np.array([0.8, 0.1, 0.0], np.float32), (SLOT + 1, 1))
        aff = np.tile(np.array([1.0, 0.0], np.float32), (SLOT + 1, 1))
        out.append(self.trc.traceNewCoarse(eye, Kt, aff))    # reads the tracer's frame
        p = self.trc.points()
        out += [np.nan_to_num(p[k], nan=-1.0) for k in sorted(p)]
        out.append(np.float64(self.ba.linearizeAll(reset=True)))
        r = self.ba.residuals()
        out += [r[k] for k in sorted(r)]
        return out

    def close(self):
        for o in (self.trk, self.trc, self.ex, self.ba):
            o.close()


def measure(case):
    calib, levels = case["calib"], case["levels"]
    w, h = calib.w_out, calib.h_out
    u = Undistorter(calib)
    f = make_select_frames(1, width=calib.w_in, height=calib.h_in, contrast_ramp=True)[0]
    raw = np.clip(np.rint(f), 0, 255).astype(np.uint8)
    scene = make_ba_scene(n_points=60, n_frames=3, width=w, height=h, seed=5, kitti=case["kitti"])
    pattern = np.random.default_rng(7).integers(-13, 14, size=(256, 2, 2), dtype=np.int8)
    lib = hip()
    im = DeviceImage(w, h, levels)
    new, par = Consumers(w, h, levels, scene, pattern), Consumers(w, h, levels, scene, pattern)

    def new_path(i):
        im.set_u8(u, raw)
        new.trk.setNewFrameImage(im, 1.0)
        new.trc.set_frame_image(im)
        new.trc.set_host_image_from(SLOT, im)
        _, n = new.sel.makeMapsImage(im, i, DENSITY, want_map=False)
        new.ex.extract_image(new.sel, im)
        new.ba.set_frame_image_from(FRAME, im)
        assert lib.hipDeviceSynchronize() == 0
        return n

    def parent_path(i):
        par.trk.setNewFrameU8(u, raw, 1.0)
        par.trc.set_frame_u8(u, raw)
        fimg, _ = u.undistort(raw, img8=False)
        _, n = par.sel.makeMapsRaw(fimg, i, DENSITY, want_map=False)
        par.trc.set_host_image(SLOT, dir_pyramid(fimg, 1)[0][0])
        par.ex.extract_u8(par.sel, u, raw)
        par.trk.frame_to_ba(par.ba, FRAME)
        assert lib.hipDeviceSynchronize() == 0
        return n

    t_new, t_par, d_new = [], [], []
    for i in range(WARMUP + ROUNDS):
        t0 = time.perf_counter()
        na = new_path(i)
        t1 = time.perf_counter()
        nb = parent_path(i)
        t2 = time.perf_counter()
        assert na == nb, (na, nb)           # both selectors walk the same potential sequence
        fused_ms = im.last_stats()          # the build alone: the hand-off's own set
        if i >= WARMUP:
            t_new.append(t1 - t0)
            t_par.append(t2 - t1)
            d_new.append(fused_ms)
    a, b = new.observe(lib, levels), par.observe(lib, levels)
    assert len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b)), \
        "the two hand-offs left different consumers"
    q = lambda v, s: [round(float(np.percentile(v, p)) * s, 1) for p in (10, 50, 90)]  # noqa: E731
    qn, qp, qf = q(t_new, 1e6), q(t_par, 1e6), q(d_new, 1e3)
    out = {"size": f"{w}x{h}", "levels": levels, "rounds": ROUNDS,
           "build_fused_us_p10_p50_p90": qf, "build_spread_us": round(qf[2] - qf[0], 1),
           "handoff_new_us_p10_p50_p90": qn, "handoff_parent_us_p10_p50_p90": qp,
           "handoff_spread_us": round(max(qn[2] - qn[0], qp[2] - qp[0]), 1), "same_consumers": True}
    for o in (new, par, im, u):
        o.close()
    return out


if __name__ == "__main__":
    lines = [json.dumps(measure(c)) for c in CASES]
    print("\n".join(lines))
    if len(sys.argv) > 2 and sys.argv[1] == "--out":
        with open(sys.argv[2], "w") as fh:
            fh.write("\n".join(lines) + "\n")
