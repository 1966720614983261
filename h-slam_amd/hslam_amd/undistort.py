"""DatasetReader::undistort (Include/DatasetLoader.h:436-506) on the device through include/hs_undist.h: the camera's
raw u8 frame in, ImageData::fImgL (and cvImgL) out; the tracker and the tracer take the raw frame directly
(CoarseTracker.setNewFrameU8, ImmatureTracer.set_frame_u8).  The two table builders run on the host, no device."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import HsError, check, hs_undist_calib, load, ptr

MODELS = {"Pinhole": 0, "Atan": 1, "RadTan": 2, "EquiDistant": 3, "KannalaBrandt": 4}
PROCESSES = {"crop": 0, "none": 1, "useK": 2}


def make_calib(model, w_in, h_in, w_out, h_out, K_in, dist=(0.0,), process="crop", desired_K=(0.0, 0.0, 0.0, 0.0)):
    """hs_undist_calib from a calibration file's fields: model / process by their names there, K_in = (fx, fy, cx, cy)
    (relative when cx < 1 and cy < 1), dist = CameraL.distM's first four (or CameraL.dist), desired_K relative."""
    c = hs_undist_calib()
    c.model, c.process = MODELS[model], PROCESSES[process]
    c.w_in, c.h_in, c.w_out, c.h_out = int(w_in), int(h_in), int(w_out), int(h_out)
    d = list(np.atleast_1d(np.asarray(dist, np.float64)))[:4]
    d += [0.0] * (4 - len(d))
    for i in range(4):
        c.K_in[i], c.dist[i], c.desired_K[i] = float(K_in[i]), float(d[i]), float(desired_K[i])
    return c


def make_remap(calib):
    """(K (4,), remap_x, remap_y (h_out, w_out)) of a calibration, on the host (hs_undist_make_remap)."""
    K = np.zeros(4, np.float32)
    rx = np.zeros((calib.h_out, calib.w_out), np.float32)
    ry = np.zeros_like(rx)
    check(load().hs_undist_make_remap(C.byref(calib), ptr(K), ptr(rx), ptr(ry)))
    return K, rx, ry


def _g256(G):
    if G is None:
        return None
    g = np.ascontiguousarray(G, np.float32).ravel()
    if g.size != 256:  # the C entry takes a bare pointer: the length is checked where it is known
        raise HsError(f"hs call failed (-1): G must have exactly 256 entries, got {g.size}")
    return g


def make_photometric(G=None, vignette=None):
    """(Binv (256,), B (256,), vignette_inv or None) on the host (hs_undist_make_photometric)."""
    g = _g256(G)
    v = None if vignette is None else np.ascontiguousarray(vignette, np.uint16)
    Binv, B = np.zeros(256, np.float32), np.zeros(256, np.float32)
    vinv = None if v is None else np.zeros(v.shape, np.float32)
    check(load().hs_undist_make_photometric(ptr(g), ptr(v), 0 if v is None else v.size, ptr(Binv), ptr(B), ptr(vinv)))
    return Binv, B, vinv


class Undistorter:
    def __init__(self, calib, device: int = 0):
        self.lib = load()
        self.calib = calib
        self.w_in, self.h_in, self.w_out, self.h_out = calib.w_in, calib.h_in, calib.w_out, calib.h_out
        h = C.c_void_p()
        check(self.lib.hs_undistorter_create(C.byref(h), device, C.byref(calib)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.hs_undistorter_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    @property
    def K(self):
        """(fx, fy, cx, cy) of the undistorted images: the K the tracker and the BA are created with."""
        k = np.zeros(4, np.float32)
        check(self.lib.hs_undistorter_get_K(self.h, ptr(k)))
        return k

    def remap(self):
        """(remap_x, remap_y), each (h_out, w_out) float32: the table in use."""
        rx = np.zeros((self.h_out, self.w_out), np.float32)
        ry = np.zeros_like(rx)
        check(self.lib.hs_undistorter_get_remap(self.h, ptr(rx), ptr(ry)))
        return rx, ry

    def set_photometric(self, G=None, vignette=None):
        """G: 256 strictly increasing response values; vignette: (h_in, w_in) u16.  Either may be None."""
        g = _g256(G)
        v = None if vignette is None else np.ascontiguousarray(vignette, np.uint16)
        assert v is None or v.shape == (self.h_in, self.w_in)
        check(self.lib.hs_undistorter_set_photometric(self.h, ptr(g), ptr(v)))

    def set_remap(self, remap_x, remap_y):
        rx = np.ascontiguousarray(remap_x, np.float32)
        ry = np.ascontiguousarray(remap_y, np.float32)
        assert rx.shape == (self.h_out, self.w_out) and ry.shape == rx.shape
        check(self.lib.hs_undistorter_set_remap(self.h, ptr(rx), ptr(ry)))

    def time_kernel(self, raw, warmup: int = 20, launches: int = 200) -> float:
        """Device milliseconds per launch of the kernel (one event pair over `launches` back-to-back launches)."""
        a = np.ascontiguousarray(raw, np.uint8)
        assert a.shape == (self.h_in, self.w_in)
        ms = C.c_float()
        check(self.lib.hs_undistorter_time_kernel(self.h, ptr(a), warmup, launches, C.byref(ms)))
        return ms.value

    def undistort(self, raw, img8: bool = True):
        """(fImg (h_out, w_out) float32, img8 (h_out, w_out) uint8 or None) of a raw (h_in, w_in) u8 frame."""
        a = np.ascontiguousarray(raw, np.uint8)
        assert a.shape == (self.h_in, self.w_in)
        f = np.zeros((self.h_out, self.w_out), np.float32)
        b = np.zeros((self.h_out, self.w_out), np.uint8) if img8 else None
        check(self.lib.hs_undistorter_apply(self.h, ptr(a), ptr(f), ptr(b)))
        return f, b
