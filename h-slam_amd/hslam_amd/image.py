"""One device-resident camera frame through include/hs_image.h: what the reference's Frame constructor builds once
per image (DirPyr, absSquaredGrad, cvImgL), uploaded, undistorted and built once and then handed to every consumer
device to device.

    im = DeviceImage(W, H, n_levels)
    im.set_u8(undistorter, raw)                  # the camera's raw (h_in, w_in) uint8 frame; returns without waiting
    im.set_raw(fImgL)                            # or ImageData::fImgL (H, W) float32: no cvImgL
    tracker.set_frame_image(im, ab_exposure)     # CoarseTracker: all levels
    tracer.set_frame_image(im)                   # ImmatureTracer: the frame to trace on
    tracer.set_host_image_from(slot, im)         # ImmatureTracer: a keyframe's DirPyr[0]
    selector.makeMapsImage(im, id, density)      # PixelSelector
    extractor.extract_image(selector, im)        # FeatureExtractor
    flow.track_image(im, 7)                      # KeypointFlow
    ba.set_frame_image_from(frame, im)           # BAWindow: hs_image_to_ba
    d, g, c = im.get(lvl, img8=True)             # parity read-back
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, load, ptr


class DeviceImage:
    def __init__(self, width: int, height: int, n_levels: int, device: int = 0):
        self.lib = load()
        self.W, self.H, self.n_levels = int(width), int(height), int(n_levels)
        h = C.c_void_p()
        check(self.lib.hs_image_create(C.byref(h), device, self.W, self.H, self.n_levels))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.hs_image_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_u8(self, undistorter, raw):
        """The frame as the camera's raw (h_in, w_in) uint8 frame (hslam_amd.undistort.Undistorter's arithmetic)."""
        a = np.ascontiguousarray(raw, np.uint8)
        if a.shape != (undistorter.h_in, undistorter.w_in):
            raise ValueError(f"raw frame must be ({undistorter.h_in}, {undistorter.w_in}), got {a.shape}")
        check(self.lib.hs_image_set_u8(self.h, undistorter.h, ptr(a)))

    def set_raw(self, fimg):
        """The frame as fImgL (H, W) float32; the image then holds no cvImgL."""
        a = np.ascontiguousarray(fimg, np.float32)
        if a.shape != (self.H, self.W):
            raise ValueError(f"image must be ({self.H}, {self.W}), got {a.shape}")
        check(self.lib.hs_image_set_raw(self.h, ptr(a)))

    def get(self, lvl: int = 0, img8: bool = False):
        """(DirPyr[lvl] (h, w, 3) float32, absSquaredGrad[lvl] (h, w) float32[, cvImgL (H, W) uint8 at level 0])."""
        w, h = self.W >> lvl, self.H >> lvl
        d, g = np.empty((h, w, 3), np.float32), np.empty((h, w), np.float32)
        c = np.empty((self.H, self.W), np.uint8) if img8 else None
        check(self.lib.hs_image_get(self.h, int(lvl), ptr(d), ptr(g), ptr(c)))
        return (d, g, c) if img8 else (d, g)

    def last_stats(self) -> float:
        """Device milliseconds of the last set's kernels."""
        ms = C.c_double()
        check(self.lib.hs_image_last_stats(self.h, C.byref(ms)))
        return ms.value
