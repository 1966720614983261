"""Host-side mirror of the initializer's DirectRefinement over the C-ABI (include/hs_refine.h).

Names follow Include/Initializer.h:108-157 / Src/Initializer.cpp:1330-2270:

    dr = DirectRefinement(scene)          # ctor: calib, frames, Pnt set-up from mvKeys / Pts3D / Triangulated
    pose, videpth, good = dr.Refine(pose) # Refine + the ctor's _Pose / _videpth write-back
    H, b, Hsc, bsc, res = dr.calcResAndGS(T, aff)   # resetPoints + one calcResAndGS (parity seam)

The initializer hand-off on the device (include/hs_init.h) starts from a refiner without frames or points:

    dr = DirectRefinement.bare(width, height, K4)
    dr.set_first_image(image, expo)       # hslam_amd.image.DeviceImage, level 0, device to device
    dr.set_second_image(image, expo)
    dr.set_points_flow(flow, tri, z)      # mvKeys from the hslam_amd.flow.KeypointFlow's FirstFramePts
    why, handles = dr.seed_window(ba, 0)  # System::InitFromInitializer's point loop into a hslam_amd.ba.BAWindow

The LM loop runs on the GPU in one workgroup (hs_k_refine); there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, load, ptr


class DirectRefinement:
    def __init__(self, scene, device: int = 0):
        self.lib = load()
        s = scene
        h = C.c_void_p()
        check(self.lib.hs_refiner_create(C.byref(h), device, s.width, s.height,
                                         ptr(np.ascontiguousarray(s.K4, np.float64))))
        self.h = h
        self.n = s.n_points
        check(self.lib.hs_refiner_set_frames(self.h, ptr(np.ascontiguousarray(s.img1, np.float32)),
                                             ptr(np.ascontiguousarray(s.img2, np.float32)),
                                             float(s.expo1), float(s.expo2)))
        self.set_points(s.u, s.v, s.tri, s.z)

    @classmethod
    def bare(cls, width: int, height: int, K4, device: int = 0):
        """A refiner of this size without frames or points (hs_refiner_create alone)."""
        self = cls.__new__(cls)
        self.lib = load()
        h = C.c_void_p()
        check(self.lib.hs_refiner_create(C.byref(h), device, int(width), int(height),
                                         ptr(np.ascontiguousarray(K4, np.float64))))
        self.h = h
        self.n = 0
        return self

    def set_frames(self, img1, img2, expo1: float = 0.0, expo2: float = 0.0):
        """Both frames from host (h, w, 3) (I, dx, dy) arrays (hs_refiner_set_frames)."""
        check(self.lib.hs_refiner_set_frames(self.h, ptr(np.ascontiguousarray(img1, np.float32)),
                                             ptr(np.ascontiguousarray(img2, np.float32)), float(expo1), float(expo2)))

    def set_first_image(self, image, ab_exposure: float = 0.0):
        """FirstFrame from level 0 of a hslam_amd.image.DeviceImage, device to device; returns without waiting."""
        check(self.lib.hs_refiner_set_first_image(self.h, image.h, float(ab_exposure)))

    def set_second_image(self, image, ab_exposure: float = 0.0):
        check(self.lib.hs_refiner_set_second_image(self.h, image.h, float(ab_exposure)))

    def set_points_flow(self, flow, tri, z):
        """The ctor's Pnt set-up with mvKeys read from the flow's FirstFramePts on the device; tri / z from the host."""
        t, zz = np.ascontiguousarray(tri, np.uint8), np.ascontiguousarray(z, np.float32)
        self.n = 0
        check(self.lib.hs_refiner_set_points_flow(self.h, flow.h, ptr(t), ptr(zz)))
        self.n = len(t)

    def set_points_twoview(self, flow, twoview):
        """The same with tri / z read on the device from the last successful fit of a hslam_amd.twoview.TwoViewFit
        (fit_flow on this flow's current first frame): z = mvIniP3D[i].z / median_depth."""
        check(self.lib.hs_refiner_set_points_twoview(self.h, flow.h, twoview.h))
        self.n = twoview.n

    def videpth(self):
        """Initializer::videpth as InitFromInitializer reads it: -1 untriangulated, the refined idepth where good,
        1 / z elsewhere."""
        out = np.zeros(self.n, np.float32)
        check(self.lib.hs_refiner_get_videpth(self.h, ptr(out)))
        return out

    def seed_window(self, ba, frame: int):
        """InitFromInitializer's point loop into window frame `frame` of a hslam_amd.ba.BAWindow, staged on the
        device.  Returns (why [n] (0 seeded, 1 no depth, 2 non-finite colour, 3 border), the seeded points' handles in
        mvKeys order); the caller's next makeIDX commits them."""
        why = np.zeros(self.n, np.uint8)
        hd = np.zeros(max(self.n, 1), np.int32)
        ns = C.c_int()
        check(self.lib.hs_refiner_seed_ba(self.h, ba.h, int(frame), ptr(why), ptr(hd), C.byref(ns)))
        return why, hd[:ns.value].copy()

    def set_points(self, u, v, tri, z):
        cols = [np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32),
                np.ascontiguousarray(tri, np.uint8), np.ascontiguousarray(z, np.float32)]
        self.n = len(cols[0])
        check(self.lib.hs_refiner_set_points(self.h, self.n, *[ptr(c) for c in cols]))

    def close(self):
        if getattr(self, "h", None):
            self.lib.hs_refiner_destroy(self.h)
            self.h = None

    __del__ = close

    def Refine(self, pose7, videpth=None):
        """Returns (refined pose, videpth with the good + triangulated points updated, isGood, iterations, snapped)."""
        T = np.array(pose7, np.float64)
        vid = np.zeros(self.n, np.float32) if videpth is None else np.array(videpth, np.float32)
        good = np.zeros(self.n, np.uint8)
        it, sn = C.c_int(), C.c_int()
        check(self.lib.hs_refiner_refine(self.h, ptr(T), ptr(vid), ptr(good), C.byref(it), C.byref(sn)))
        return T, vid, good, it.value, bool(sn.value)

    def calcResAndGS(self, T7, aff=(0.0, 0.0)):
        H, Hs = np.zeros(64, np.float32), np.zeros(64, np.float32)
        b, bs, res = np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(3, np.float32)
        check(self.lib.hs_refiner_calc_res(self.h, ptr(np.ascontiguousarray(T7, np.float64)),
                                           ptr(np.ascontiguousarray(aff, np.float64)),
                                           ptr(H), ptr(b), ptr(Hs), ptr(bs), ptr(res)))
        return H.reshape(8, 8), b, Hs.reshape(8, 8), bs, res

    def log(self):
        out = np.zeros((1001, 8), np.float32)
        n = self.lib.hs_refiner_get_log(self.h, 1001, ptr(out))
        if n < 0:
            check(n)
        return out[:n]

    def points(self):
        f7 = np.zeros((self.n, 7), np.float32)
        g2 = np.zeros((self.n, 2), np.uint8)
        jb = np.zeros((self.n, 10), np.float32)
        check(self.lib.hs_refiner_get_points(self.h, ptr(f7), ptr(g2), ptr(jb)))
        return dict(idepth=f7[:, 0], idepth_new=f7[:, 1], iR=f7[:, 2], energy_new0=f7[:, 3], energy_new1=f7[:, 4],
                    maxstep=f7[:, 5], lastHessian_new=f7[:, 6], isGood=g2[:, 0], isGood_new=g2[:, 1], jb_new=jb)

    def last_ms(self) -> float:
        t = np.zeros(1)
        check(self.lib.hs_refiner_last_ms(self.h, ptr(t)))
        return float(t[0])
