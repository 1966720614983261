"""The device-resident map of the points that left the BA window (include/hs_map.h): what the reference keeps in
Frame::pointHessiansMarginalized / pointHessiansOut, KFDisplay::RefreshPC over it, and the settings of
System::flagFramesForMarginalization.

    m = PointMap.create(capacity)          # hs_map_create
    ba.attachMap(m)                        # hs_ba_attach_map: the window's removals append records
    m.records()                            # structured array of hs_map_record
    m.frame_counts(frame_id)               # (pointHessiansMarginalized.size(), pointHessiansOut.size())
    m.refresh_cloud(frame_id, ba)          # KFDisplay::RefreshPC for one keyframe
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import check, hs_frame_marg_params, load, ptr

PT_OUTLIER, PT_MARGINALIZED = 1, 3  # the reference's PtStatus values of a retired point

RECORD = np.dtype([("handle", np.int32), ("frame_id", np.int32), ("status", np.int32),
                   ("numGoodResiduals", np.int32), ("u", np.float32), ("v", np.float32), ("idepth", np.float32),
                   ("idepth_zero", np.float32), ("hdif", np.float32), ("maxRelBaseline", np.float32),
                   ("color", np.uint8, 8), ("reserved", np.uint8, 16)])
assert RECORD.itemsize == 64


def frame_marg_params(**over):
    """hs_frame_marg_params with the reference's settings (Src/Settings.cpp:52-59), fields overridden by keyword."""
    p = hs_frame_marg_params()
    check(load().hs_frame_marg_params_default(C.byref(p)))
    for k, v in over.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class PointMap:
    def __init__(self, capacity: int, device: int = 0):
        self.lib = load()
        h = C.c_void_p()
        check(self.lib.hs_map_create(C.byref(h), int(capacity), int(device)))
        self.h = h
        self.capacity = int(capacity)

    @classmethod
    def create(cls, capacity: int, device: int = 0) -> "PointMap":
        return cls(capacity, device)

    def size(self):
        """(records, keyframes with at least one record)."""
        n, f = C.c_int(), C.c_int()
        check(self.lib.hs_map_size(self.h, C.byref(n), C.byref(f)))
        return n.value, f.value

    def __len__(self):
        return self.size()[0]

    def frame_counts(self, frame_id: int):
        """(n_marginalized, n_out) of the keyframe with hs_frame.id frame_id (host-side counters)."""
        a, b = C.c_int(), C.c_int()
        check(self.lib.hs_map_frame_counts(self.h, int(frame_id), C.byref(a), C.byref(b)))
        return a.value, b.value

    def records(self, first: int = 0, n: int | None = None):
        """Records [first, first + n) in push order as a structured array (dtype RECORD)."""
        if n is None:
            n = len(self) - first
        out = np.zeros(max(n, 0), RECORD)
        check(self.lib.hs_map_get_records(self.h, int(first), int(n), ptr(out)))
        return out

    def clear(self):
        check(self.lib.hs_map_clear(self.h))

    def refresh_cloud(self, frame_id: int, ba, cap: int | None = None):
        """KFDisplay::RefreshPC for one keyframe: dict(xyz [n, 3] float32, rgb [n, 3] uint8, n, kinv (fxi, fyi, cxi,
        cyi)).  ba: the BAWindow whose committed window may still hold the frame, and whose calibration is used."""
        cap = self.capacity * 8 if cap is None else int(cap)
        xyz, rgb = np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.uint8)
        n, kinv = C.c_int(), np.zeros(4, np.float32)
        check(self.lib.hs_map_refresh_cloud(self.h, ba.h, int(frame_id), ptr(xyz), ptr(rgb),
                                            cap, C.byref(n), ptr(kinv)))
        k = min(n.value, cap)
        return dict(xyz=xyz[:k].copy(), rgb=rgb[:k].copy(), n=n.value, kinv=kinv)

    def cloud_device(self):
        """(device address of the vertices, of the colours, vertex count) of the last refresh."""
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_int()
        check(self.lib.hs_map_cloud_device(self.h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.hs_map_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()
