"""Frame::Extract -> FeatureDetector::ExtractFeatures (Src/Detector.cpp:31-131, UseFAST = false, DoSubPix = false) on
the device through include/hs_extract.h: the keys of a selection map's interior in raster order, the 7x7 blur of
cvImgL, and each key's intensity-centroid angle and 256-bit rotated-BRIEF descriptor.

    ex = FeatureExtractor(W, H, capacity, pattern)        # pattern: FeatureDetector::pattern, (256, 2, 2) int8 in +-13
    n = ex.extract(selectionMap, cvImgL)                   # host map and image
    n = ex.extract_selected(selector, cvImgL)              # the map of selector's last makeMaps, read on the device
    n = ex.extract_u8(selector, undistorter, raw)          # cvImgL made from the camera's raw frame on the device
    n = ex.extract_image(selector, image)                  # cvImgL of a DeviceImage (hslam_amd.image), on the device
    r = ex.get()                                           # dict(xy, angle, desc[, blurred])
    tracer.add_keys(ex, slot)                              # makeNewTraces: one ImmaturePoint per key, device to device
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import HsError, check, load, ptr

BORDER = 19        # keys lie in [19, W-19) x [19, H-19)
PATTERN_MAX = 13   # |pattern entry| <= 13


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
