"""Tracing against the BA window (hs_tracer_trace_ba), the parts that need no GPU: the entry points exist, and the
per-host traceOn arguments the device forms from the window's frames (hs_host_math.h make_trace_host, run here on the
host through hs_debug_trace_hosts) against an fp64 evaluation of Src/Mapping.cpp:500-513."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
EPS64 = 2.0 ** -53
F32 = np.float32


def test_header_declares_and_library_exports_the_entry_points():
    from hslam_amd import _lib
    from hslam_amd.trace import ImmatureTracer
    hdr = open(os.path.join(ROOT, "include", "hs_trace.h")).read()
    lib = _lib.load()
    for name in ("hs_tracer_trace_ba", "hs_tracer_get_trace_inputs"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert "hs_debug_trace_hosts" in _lib.SIGNATURES and getattr(lib, "hs_debug_trace_hosts") is not None
    assert callable(ImmatureTracer.trace_ba) and callable(ImmatureTracer.trace_inputs)
    # hs_tracer_trace stays
    assert re.search(r"\bint\s+hs_tracer_trace\s*\(", hdr)


def _quat_rot(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def trace_hosts(w2c, aff, expo, K4, new_w2c, new_aff, new_expo):
    """hs_debug_trace_hosts over planted frames -> [nF, 14] float32 (KRKi | Kt | aff)."""
    from hslam_amd import _lib
    nF = len(w2c)
    out = np.zeros((nF, 14), np.float32)
    a = [np.ascontiguousarray(w2c, np.float64), np.ascontiguousarray(aff, np.float64),
         np.ascontiguousarray(expo, np.float32), np.ascontiguousarray(K4, np.float32),
         np.ascontiguousarray(new_w2c, np.float64), np.ascontiguousarray(new_aff, np.float64)]
    _lib.check(_lib.load().hs_debug_trace_hosts(None, nF, None, *[_lib.ptr(x) for x in a], float(new_expo),
                                                _lib.ptr(out)))
    return out


def inverse_f32(K):
    """Mat33f::inverse() as Eigen computes it (cofactors, determinant, one reciprocal), every operation in float."""
    M = K.astype(F32)

    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return F32(F32(M[i1, j1] * M[i2, j2]) - F32(M[i1, j2] * M[i2, j1]))

    c = [cof(0, 0), cof(1, 0), cof(2, 0)]
    det = F32(F32(F32(c[0] * M[0, 0]) + F32(c[1] * M[1, 0])) + F32(c[2] * M[2, 0]))
    inv = F32(F32(1.0) / det)
    return np.array([[c[0] * inv, c[1] * inv, c[2] * inv],
                     [cof(0, 1) * inv, cof(1, 1) * inv, cof(2, 1) * inv],
                     [cof(0, 2) * inv, cof(1, 2) * inv, cof(2, 2) * inv]], F32)


def planted(seed):
    rng = np.random.default_rng(300 + seed)
    nF = 8
    q = rng.normal(size=(nF + 1, 4)) * [0.05, 0.05, 0.05, 0] + [0, 0, 0, 1]
    t = rng.normal(size=(nF + 1, 3)) * 0.3
    w2c = np.concatenate([q, t], 1)
    aff = np.stack([rng.uniform(-0.05, 0.05, nF + 1), rng.uniform(-5, 5, nF + 1)], 1)
    expo = rng.uniform(0.5, 2.0, nF + 1).astype(np.float32)
    K4 = np.array([[256.0, 254.4, 319.5, 239.5], [718.856, 718.856, 615.5, 183.5], [128.3, 127.9, 161.2, 118.7]][seed],
                  np.float32)
    return w2c, aff, expo, K4


def check_against_fp64(got, w2c, aff, expo, K4, new_expo):
    """Rows 0 .. nF-1 of the planted frames are the hosts, the last row the new frame."""
    nF = len(w2c) - 1
    fx, fy, cx, cy = (float(v) for v in K4)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    Ki = inverse_f32(K)
    assert np.all(np.abs(Ki - np.linalg.inv(K)) <= 5 * EPS * np.abs(np.linalg.inv(K)))
    Kid = Ki.astype(np.float64)
    Rn, tn = _quat_rot(w2c[nF, :4]), w2c[nF, 4:]
    for h in range(nF):
        Rh, th = _quat_rot(w2c[h, :4]), w2c[h, 4:]
        R = Rn @ Rh.T
        tr = tn - R @ th
        # hostToNew is an fp64 product, formed by quaternions in the library and by matrices here (test_act_ba.py)
        dR = 16 * EPS64 * (np.abs(Rn) @ np.abs(Rh.T))
        dt = 16 * EPS64 * (np.abs(tn) + np.abs(R) @ np.abs(th))
        ref = K @ R @ Kid
        bound = 8 * EPS * (np.abs(K) @ np.abs(R) @ np.abs(Kid)) + np.abs(K) @ dR @ np.abs(Kid)
        assert np.all(np.abs(got[h, :9].reshape(3, 3) - ref) <= bound), h
        bound = 8 * EPS * (np.abs(K) @ np.abs(tr)) + np.abs(K) @ dt
        assert np.all(np.abs(got[h, 9:12] - K @ tr) <= bound), h
        eF, eT = float(expo[h]), float(new_expo)
        if eF == 0 or eT == 0:
            eF = eT = 1.0
        a = np.exp(aff[nF, 0] - aff[h, 0]) * eT / eF
        b = aff[nF, 1] - a * aff[h, 1]
        assert abs(float(got[h, 12]) - a) <= np.spacing(F32(abs(a))), h
        assert abs(float(got[h, 13]) - b) <= np.spacing(F32(abs(b))), h


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_formed_hosts_against_fp64(seed):
    """KRKi = K R K^-1 and Kt = K t with the level-0 K in float: every entry within 8 x 2^-24 x the same product
    formed from absolute values (test_act_ba.py's bar for the same nested three-term float sums); aff =
    fromToVecExposure(host, new) within one float ulp."""
    w2c, aff, expo, K4 = planted(seed)
    nF = len(w2c) - 1
    got = trace_hosts(w2c[:nF], aff[:nF], expo[:nF], K4, w2c[nF], aff[nF], expo[nF])
    assert np.all(aff[:, 0] != 0) and np.all(aff[:, 1] != 0) and len(set(expo.tolist())) == nF + 1
    check_against_fp64(got, w2c, aff, expo, K4, expo[nF])
    # the eF == 0 || eT == 0 rule: both exposures count as 1 -- one host without an exposure, then the new frame
    e0 = expo.copy()
    e0[3] = 0
    got0 = trace_hosts(w2c[:nF], aff[:nF], e0[:nF], K4, w2c[nF], aff[nF], e0[nF])
    check_against_fp64(got0, w2c, aff, e0, K4, e0[nF])
    assert got0[3, 12] != got[3, 12]
    assert np.array_equal(np.delete(got0, 3, 0), np.delete(got, 3, 0))
    gotn = trace_hosts(w2c[:nF], aff[:nF], expo[:nF], K4, w2c[nF], aff[nF], 0.0)
    check_against_fp64(gotn, w2c, aff, expo, K4, 0.0)
    assert np.all(gotn[:, 12] != got[:, 12]) and np.array_equal(gotn[:, :12], got[:, :12])


def test_K_is_the_level_0_matrix():
    """traceNewCoarse's K (Src/Mapping.cpp:500-504) is CalibData's level-0 matrix on both sides of R; activation's
    K[1] R Ki[0] (CoarseDistanceMap::makeK) is another one.  With fx[1] = fx / 2 and cx[1] = (cx + 0.5) / 2 - 0.5 the
    two differ in every row but the last, so the level-0 evaluation passes and the level-1 one is far off."""
    from test_act_ba import formed_inputs
    w2c, aff, expo, K4 = planted(0)
    nF = len(w2c) - 1
    got = trace_hosts(w2c[:nF], aff[:nF], expo[:nF], K4, w2c[nF], aff[nF], expo[nF])
    check_against_fp64(got, w2c, aff, expo, K4, expo[nF])
    # the activation's records of the same frames with the new frame as the newest: level 1
    # (a window of 8: hosts 1 .. 7 and the new frame)
    fr, _, K1, _ = formed_inputs(w2c[1:], aff[1:], expo[1:], K4)
    assert K1[0, 0] == F32(float(K4[0]) * 0.5) and K1[0, 0] != K4[0]
    for h in range(1, nF):
        # (K R K^-1)[0, 0] = R00 + cx R20 / fx and (K[1] R Ki[0])[0, 0] = R00 / 2 + cx[1] R20 / fx: the first is twice
        # the second up to (cx - 2 cx[1]) R20 / fx = R20 / (2 fx), and |R20| <= 1
        l0, l1 = got[h, :9].reshape(3, 3), fr[h - 1]["KRKi"].reshape(3, 3)
        assert l0[0, 0] > 0.5 and l0[1, 1] > 0.5
        assert abs(l0[0, 0] - 2 * l1[0, 0]) <= 0.5 / float(K4[0]) + 1e-5
        assert abs(l0[1, 1] - 2 * l1[1, 1]) <= 0.5 / float(K4[1]) + 1e-5
    # and K^-1 on the right is K's own inverse: a pure rotation about the optical axis keeps the principal point
    q = np.array([0, 0, np.sin(0.1), np.cos(0.1), 0, 0, 0.0])
    ident = np.array([[0, 0, 0, 1.0, 0, 0, 0]])
    g = trace_hosts(ident, [[0.0, 0.0]], [1.0], K4, q, [0.0, 0.0], 1.0)[0]
    c = np.array([float(K4[2]), float(K4[3]), 1.0])
    assert np.allclose(g[:9].reshape(3, 3).astype(np.float64) @ c, c, rtol=1e-5)
    assert g[12] == 1.0 and g[13] == 0.0 and np.all(g[9:12] == 0)
