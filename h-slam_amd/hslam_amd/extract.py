"""Frame::Extract -> FeatureDetector::ExtractFeatures (Src/Detector.cpp:31-131, UseFAST = false, DoSubPix = false) on
the device through include/hs_extract.h: the keys of a selection map's interior in raster order, the 7x7 blur of
cvImgL, and each key's intensity-centroid angle and 256-bit rotated-BRIEF descriptor.

    ex = FeatureExtractor(W, H, capacity, pattern)        # pattern: FeatureDetector::pattern, (256, 2, 2) int8 in +-13
    n = ex.extract(selectionMap, cvImgL)                   # host map and image
    n = ex.extract_selected(selector, cvImgL)              # the map of selector's last makeMaps, read on the device
    n = ex.extract_u8(selector, undistorter, raw)          # cvImgL made from the camera's raw frame on the device
    n = ex.extract_image(selector, image)                  # cvImgL of a DeviceImage (hslam_amd.image), on the device
    n = ex.extract_fast(cvImgL, fast_params(threshold=8))  # UseFAST = true: cv::FAST + Ssc pick the keys
    n = ex.extract_fast_u8(undistorter, raw)               #   (also extract_fast_image(image))
    f = ex.get_fast()                                      # dict(n_corners, width, response, corner_xy, corner_response)
    r = ex.get()                                           # dict(xy, angle, desc[, blurred])
    tracer.add_keys(ex, slot)                              # makeNewTraces: one ImmaturePoint per key, device to device
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import HsError, check, hs_fast_params, load, ptr

BORDER = 19        # keys lie in [19, W-19) x [19, H-19)
PATTERN_MAX = 13   # |pattern entry| <= 13


def fast_params(**kw):
    """hs_fast_params with the reference's settings (threshold 8, num_features 3000, min_dist 5, tolerance 0.1),
    fields overridden by keyword."""
    p = hs_fast_params()
    load().hs_fast_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in ("threshold", "num_features", "min_dist", "tolerance"):
            raise TypeError(f"hs_fast_params has no field {k!r}")
        setattr(p, k, v)
    return p


class ExtractOverflow(HsError):
    """An extract found more keys than the extractor's capacity; ``needed`` is the count.  Nothing was truncated and
    the previous result is still the one ``get`` returns."""

    def __init__(self, msg, needed):
        super().__init__(msg)
        self.needed = needed


class FeatureExtractor:
    def __init__(self, width: int, height: int, capacity: int, pattern, device: int = 0):
        self.lib = load()
        self.W, self.H, self.capacity = int(width), int(height), int(capacity)
        pat = np.ascontiguousarray(pattern, np.int8).ravel()
        if pat.size != 1024:  # the C entry takes a bare pointer: the length is checked where it is known
            raise HsError(f"hs call failed (-1): pattern must have 256 x 2 x 2 entries, got {pat.size}")
        h = C.c_void_p()
        check(self.lib.hs_extractor_create(C.byref(h), device, self.W, self.H, self.capacity, ptr(pat)))
        self.h = h
        self.n = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.hs_extractor_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _done(self, rc, n):
        if rc == -1 and n.value > self.capacity:
            raise ExtractOverflow(f"hs call failed ({rc}): {self.lib.hs_last_error().decode(errors='replace')}", n.value)
        check(rc)
        self.n = n.value
        return self.n

    def _img(self, img8, shape=None):
        a = np.ascontiguousarray(img8, np.uint8)
        shape = shape or (self.H, self.W)
        if a.shape != shape:
            raise ValueError(f"image must be {shape}, got {a.shape}")
        return a

    def extract(self, selection_map, img8) -> int:
        """ExtractFeatures on a host selection map (H, W) float32 and cvImgL (H, W) uint8; returns mvKeys.size()."""
        m = np.ascontiguousarray(selection_map, np.float32)
        if m.shape != (self.H, self.W):
            raise ValueError(f"map must be ({self.H}, {self.W}), got {m.shape}")
        a = self._img(img8)
        n = C.c_int()
        return self._done(self.lib.hs_extractor_extract(self.h, ptr(m), ptr(a), C.byref(n)), n)

    def extract_selected(self, selector, img8) -> int:
        """The same on the map of ``selector``'s (PixelSelector) last makeMaps, where it lies on the device."""
        a = self._img(img8)
        n = C.c_int()
        return self._done(self.lib.hs_extractor_extract_selected(self.h, selector.h, ptr(a), C.byref(n)), n)

    def extract_u8(self, selector, undistorter, raw) -> int:
        """The same, cvImgL being the undistorter's 8-bit output of the camera's raw (h_in, w_in) frame."""
        a = self._img(raw, (undistorter.h_in, undistorter.w_in))
        n = C.c_int()
        return self._done(self.lib.hs_extractor_extract_u8(self.h, selector.h, undistorter.h, ptr(a), C.byref(n)), n)

    def extract_image(self, selector, image) -> int:
        """The same, cvImgL being that of a hslam_amd.image.DeviceImage set from a raw u8 frame, read on the device."""
        n = C.c_int()
        return self._done(self.lib.hs_extractor_extract_image(self.h, selector.h, image.h, C.byref(n)), n)

    # ---- the UseFAST = true branch: cv::FAST 9-16 with suppression, the sort by response, Ssc and its final pass

    def _fast(self, params):
        if params is None:
            return fast_params()
        if isinstance(params, dict):
            return fast_params(**params)
        return params

    def extract_fast(self, img8, params=None) -> int:
        """ExtractFeatures with UseFAST = true on cvImgL (H, W) uint8; params: fast_params(...), a dict of its
        fields, or None for the reference's settings.  Returns mvKeys.size()."""
        a = self._img(img8)
        p = self._fast(params)
        n = C.c_int()
        return self._done(self.lib.hs_extractor_extract_fast(self.h, C.byref(p), ptr(a), C.byref(n)), n)

    def extract_fast_u8(self, undistorter, raw, params=None) -> int:
        """The same, cvImgL being the undistorter's 8-bit output of the camera's raw (h_in, w_in) frame."""
        a = self._img(raw, (undistorter.h_in, undistorter.w_in))
        p = self._fast(params)
        n = C.c_int()
        return self._done(self.lib.hs_extractor_extract_fast_u8(self.h, C.byref(p), undistorter.h, ptr(a), C.byref(n)), n)

    def extract_fast_image(self, image, params=None) -> int:
        """The same, cvImgL being that of a hslam_amd.image.DeviceImage set from a raw u8 frame, read on the device."""
        p = self._fast(params)
        n = C.c_int()
        return self._done(self.lib.hs_extractor_extract_fast_image(self.h, C.byref(p), image.h, C.byref(n)), n)

    def get_fast(self):
        """The last fast extract: dict(n_corners = corners before Ssc, width = the Ssc width whose result was taken
        (-1: none evaluated), response (n,) float32 = mvKeys[i].response, corner_xy (n_corners, 2) and
        corner_response (n_corners,) float32 in sorted order).  HsError (-5) unless the current result is a fast
        extract's."""
        nc, w = C.c_int(), C.c_int()
        check(self.lib.hs_extractor_get_fast(self.h, C.byref(nc), C.byref(w), None, None, None))
        n = C.c_int()
        check(self.lib.hs_extractor_get(self.h, C.byref(n), None, None, None, None))
        out = dict(n_corners=nc.value, width=w.value, response=np.zeros(n.value, np.float32),
                   corner_xy=np.zeros((nc.value, 2), np.float32), corner_response=np.zeros(nc.value, np.float32))
        check(self.lib.hs_extractor_get_fast(self.h, None, None, ptr(out["response"]), ptr(out["corner_xy"]),
                                             ptr(out["corner_response"])))
        return out

    def fast_widths(self):
        """Debug read of the last fast extract's Ssc search: dict(low, high, taken = {width: int32 array of the
        sorted corner indices that width took, in order}) for every width of [low, high]."""
        n = self.get_fast()["n_corners"]
        lo, hi, c = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.hs_debug_fast_width(self.h, 0, C.byref(lo), C.byref(hi), C.byref(c), None, 0))
        taken = {}
        for w in range(lo.value, hi.value + 1):
            buf = np.zeros(max(n, 1), np.int32)
            check(self.lib.hs_debug_fast_width(self.h, w, C.byref(lo), C.byref(hi), C.byref(c), ptr(buf), n))
            taken[w] = buf[:c.value].copy() if c.value >= 0 else None
        return dict(low=lo.value, high=hi.value, taken=taken)

    def get(self, blurred: bool = False):
        """The last successful extract: dict(xy (n, 2) float32 = mvKeys[i].pt, angle (n,) float32 degrees,
        desc (n, 32) uint8[, blurred (H, W) uint8 = ImageBlurred])."""
        n = C.c_int()
        check(self.lib.hs_extractor_get(self.h, C.byref(n), None, None, None, None))
        m = n.value
        out = dict(xy=np.zeros((m, 2), np.float32), angle=np.zeros(m, np.float32), desc=np.zeros((m, 32), np.uint8))
        b = np.zeros((self.H, self.W), np.uint8) if blurred else None
        check(self.lib.hs_extractor_get(self.h, C.byref(n), ptr(out["xy"]), ptr(out["angle"]), ptr(out["desc"]), ptr(b)))
        if blurred:
            out["blurred"] = b
        return out

    def last_stats(self) -> float:
        """Device milliseconds of the last extract's kernels."""
        ms = C.c_double()
        check(self.lib.hs_extractor_last_stats(self.h, C.byref(ms)))
        return ms.value
