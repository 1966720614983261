"""Initializer::FindMatches (Src/Initializer.cpp:341-399) on the device through include/hs_flow.h: pyramidal
Lucas-Kanade flow (15 x 15 window, maxLevel 2, 30 iterations / eps 0.01) of the first frame's keypoints into every
later frame, with the reference's bookkeeping of previous points, outputs and good flags.

    fl = KeypointFlow(W, H, capacity)
    fl.set_first(cvImgL, xy)                     # Initialize()'s first-frame branch; or
    n = fl.set_first_extracted(extractor)        # cvImgL and the keys where the extractor's last extract left them
    n_good = fl.track(cvImgL, 7)                 # one FindMatches; or
    n_good = fl.track_extracted(extractor, 7)    # the new frame's cvImgL where the extractor left it; or
    n_good = fl.track_u8(undistorter, raw, 7)    # cvImgL made from the camera's raw frame on the device
    n_good = fl.track_image(image, 7)            # cvImgL of a DeviceImage (hslam_amd.image), on the device
    r = fl.get()                                 # dict(first_xy, prev_xy, xy, status, err, good)
    m = fl.mean_flow()                           # ComputeMeanOpticalFlow(MatchedPtsBkp, MatchedPts), on the host
    m = fl.mean_flow_device()                    # the same 4 bytes made on the device
    r = fl.calc(prev8, next8, prev_xy[, init_xy])  # one stand-alone calcOpticalFlowPyrLK: dict(xy, status, err)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, load, ptr

WIN = 15
MAX_LEVEL = 2


class KeypointFlow:
    def __init__(self, width: int, height: int, capacity: int, device: int = 0):
        self.lib = load()
        self.W, self.H, self.capacity = int(width), int(height), int(capacity)
        h = C.c_void_p()
        check(self.lib.hs_flow_create(C.byref(h), device, self.W, self.H, self.capacity))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.hs_flow_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _img(self, img8, shape=None):
        a = np.ascontiguousarray(img8, np.uint8)
        shape = shape or (self.H, self.W)
        if a.shape != shape:
            raise ValueError(f"image must be {shape}, got {a.shape}")
        return a

    @staticmethod
    def _pts(xy):
        a = np.ascontiguousarray(xy, np.float32)
        if a.ndim != 2 or a.shape[1] != 2:
            a = a.reshape(-1, 2)
        return a

    def set_first(self, img8, xy) -> int:
        """The first frame: cvImgL (H, W) uint8 and its keypoints (n, 2) float32."""
        a, p = self._img(img8), self._pts(xy)
        check(self.lib.hs_flow_set_first(self.h, ptr(a), len(p), ptr(p)))
        return len(p)

    def set_first_extracted(self, extractor) -> int:
        """The same from ``extractor``'s (FeatureExtractor) last extract, device to device; returns the key count."""
        n = C.c_int()
        check(self.lib.hs_flow_set_first_extracted(self.h, extractor.h, C.byref(n)))
        return n.value

    def set_first_image(self, image, xy) -> int:
        """The first frame with cvImgL from a hslam_amd.image.DeviceImage, device to device, and host keypoints."""
        p = self._pts(xy)
        check(self.lib.hs_flow_set_first_image(self.h, image.h, len(p), ptr(p)))
        return len(p)

    def track(self, img8, max_l1_error: float) -> int:
        """One FindMatches against the new frame's cvImgL; returns the number of good points."""
        a = self._img(img8)
        n = C.c_int()
        check(self.lib.hs_flow_track(self.h, ptr(a), max_l1_error, C.byref(n)))
        return n.value

    def track_extracted(self, extractor, max_l1_error: float) -> int:
        n = C.c_int()
        check(self.lib.hs_flow_track_extracted(self.h, extractor.h, max_l1_error, C.byref(n)))
        return n.value

    def track_u8(self, undistorter, raw, max_l1_error: float) -> int:
        a = self._img(raw, (undistorter.h_in, undistorter.w_in))
        n = C.c_int()
        check(self.lib.hs_flow_track_u8(self.h, undistorter.h, ptr(a), max_l1_error, C.byref(n)))
        return n.value

    def track_image(self, image, max_l1_error: float) -> int:
        """One FindMatches against the cvImgL of a hslam_amd.image.DeviceImage set from a raw u8 frame."""
        n = C.c_int()
        check(self.lib.hs_flow_track_image(self.h, image.h, max_l1_error, C.byref(n)))
        return n.value

    def get(self):
        """dict(first_xy, prev_xy (MatchedPtsBkp), xy (MatchedPts): (n, 2) float32; status, good (MatchedStatus): (n,)
        uint8; err: (n,) float32) of the last track."""
        n = C.c_int()
        check(self.lib.hs_flow_get(self.h, C.byref(n), *([None] * 6)))
        m = n.value
        out = dict(first_xy=np.zeros((m, 2), np.float32), prev_xy=np.zeros((m, 2), np.float32),
                   xy=np.zeros((m, 2), np.float32), status=np.zeros(m, np.uint8), err=np.zeros(m, np.float32),
                   good=np.zeros(m, np.uint8))
        check(self.lib.hs_flow_get(self.h, C.byref(n), ptr(out["first_xy"]), ptr(out["prev_xy"]), ptr(out["xy"]),
                                   ptr(out["status"]), ptr(out["err"]), ptr(out["good"])))
        return out

    def mean_flow(self) -> np.float32:
        m = C.c_float()
        check(self.lib.hs_flow_mean_flow(self.h, C.byref(m)))
        return np.float32(m.value)

    def mean_flow_device(self) -> np.float32:
        """mean_flow()'s value made on the device: only the result is read back."""
        m = C.c_float()
        check(self.lib.hs_flow_mean_flow_device(self.h, C.byref(m)))
        return np.float32(m.value)

    def calc(self, prev8, next8, prev_xy, init_xy=None):
        """One calcOpticalFlowPyrLK between two images for the given points; the tracked state is not touched."""
        a, b, p = self._img(prev8), self._img(next8), self._pts(prev_xy)
        g = None
        if init_xy is not None:
            g = self._pts(init_xy)
            if g.shape != p.shape:
                raise ValueError(f"init_xy must be {p.shape}, got {g.shape}")
        n = len(p)
        out = dict(xy=np.zeros((n, 2), np.float32), status=np.zeros(n, np.uint8), err=np.zeros(n, np.float32))
        check(self.lib.hs_flow_calc(self.h, ptr(a), ptr(b), n, ptr(p), ptr(g), ptr(out["xy"]), ptr(out["status"]),
                                    ptr(out["err"])))
        return out

    def pyramid(self, which: int, level: int):
        """(img (h, w) uint8, deriv (h, w, 2) int16) of a level of the last calc's / track's previous (0) or next
        (1) image."""
        w, h = C.c_int(), C.c_int()
        check(self.lib.hs_flow_get_pyramid(self.h, which, level, None, None, C.byref(w), C.byref(h)))
        img = np.zeros((h.value, w.value), np.uint8)
        deriv = np.zeros((h.value, w.value, 2), np.int16)
        check(self.lib.hs_flow_get_pyramid(self.h, which, level, ptr(img), ptr(deriv), None, None))
        return img, deriv

    def last_stats(self):
        """(device ms, Lucas-Kanade iterations run, levels) of the last calc / track."""
        ms, it, lv = C.c_double(), C.c_longlong(), C.c_int()
        check(self.lib.hs_flow_last_stats(self.h, C.byref(ms), C.byref(it), C.byref(lv)))
        return ms.value, it.value, lv.value
