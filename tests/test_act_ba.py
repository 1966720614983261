"""Point activation into the BA window (hs_tracer_activate_ba), the parts that need no GPU: the entry points exist,
the per-frame / per-pair inputs the device forms from the window's poses (hs_host_math.h make_act_*, run here on the
host through hs_debug_act_inputs) against an fp64 evaluation, the host mirror's rule for the activated points against
hs_ba_insert_points + hs_ba_insert_residuals, and the scene the GPU tests stand on."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
EPS64 = 2.0 ** -53
IN, OOB = 0, 1


def test_header_declares_and_library_exports_the_entry_points():
    from hslam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hs_trace.h")).read()
    lib = _lib.load()
    for name in ("hs_tracer_activate_ba", "hs_tracer_compact_device", "hs_tracer_get_act_inputs"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    for name in ("hs_debug_act_inputs", "hs_debug_act_mirror"):
        assert getattr(lib, name) is not None
    # hs_tracer_compact stays
    assert re.search(r"\bint\s+hs_tracer_compact\s*\(", hdr)


def _quat_rot(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def formed_inputs(w2c, aff, expo, K4):
    from hslam_amd import _lib
    from hslam_amd.trace import ACT_FRAME_DT, ACT_PAIR_DT
    nF = len(w2c)
    fr, pr, kk = np.zeros(nF, ACT_FRAME_DT), np.zeros(nF * nF, ACT_PAIR_DT), np.zeros(18, np.float32)
    a = [np.ascontiguousarray(w2c, np.float64), np.ascontiguousarray(aff, np.float64),
         np.ascontiguousarray(expo, np.float32), np.ascontiguousarray(K4, np.float32)]
    _lib.check(_lib.load().hs_debug_act_inputs(None, nF, *[_lib.ptr(x) for x in a], _lib.ptr(fr), _lib.ptr(pr),
                                               _lib.ptr(kk)))
    return fr, pr, kk[:9].reshape(3, 3), kk[9:].reshape(3, 3)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_formed_inputs_against_fp64(seed):
    """KRKi = K[1] R Ki[0], Kt = K[1] t, PRE_RTll / PRE_tTll / PRE_aff_mode: every entry within 8 x 2^-24 x the same
    product formed from absolute values (the forward bound of two nested three-term float products plus the casts)."""
    rng = np.random.default_rng(100 + seed)
    nF = 8
    q = rng.normal(size=(nF, 4)) * [0.05, 0.05, 0.05, 0] + [0, 0, 0, 1]
    t = rng.normal(size=(nF, 3)) * 0.3
    w2c = np.concatenate([q, t], 1)
    aff = np.stack([rng.uniform(-0.05, 0.05, nF), rng.uniform(-5, 5, nF)], 1)
    expo = rng.uniform(0.5, 2.0, nF).astype(np.float32)
    K4 = np.array([[256.0, 254.4, 319.5, 239.5], [718.856, 718.856, 615.5, 183.5], [128.3, 127.9, 161.2, 118.7]][seed],
                  np.float32)
    fr, pr, K1, Ki0 = formed_inputs(w2c, aff, expo, K4)
    # CoarseDistanceMap::makeK: level 1 in float from double expressions; Ki[0] = K[0]^-1 in float (cofactors,
    # determinant, reciprocal, product: 4 roundings)
    fx, fy, cx, cy = (float(v) for v in K4)
    assert K1[0, 0] == np.float32(fx * 0.5) and K1[1, 1] == np.float32(fy * 0.5)
    assert K1[0, 2] == np.float32((cx + 0.5) / 2 - 0.5) and K1[1, 2] == np.float32((cy + 0.5) / 2 - 0.5)
    Ki_ref = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]))
    assert np.all(np.abs(Ki0 - Ki_ref) <= 5 * EPS * np.abs(Ki_ref))
    K1d, Kid = K1.astype(np.float64), Ki0.astype(np.float64)
    Rs = [_quat_rot(w2c[f, :4]) for f in range(nF)]
    new = nF - 1
    for h in range(nF):
        for tg in range(nF):
            R = Rs[tg] @ Rs[h].T
            tr = t[tg] - R @ t[h]
            # fhToNew itself is an fp64 product, formed by quaternions in the library and by matrices here: two
            # evaluations of one quantity, each within 16 x 2^-53 x the sum of its terms' magnitudes (this matters
            # only where the terms cancel, as in the translation of a frame onto itself)
            dR = 16 * EPS64 * (np.abs(Rs[tg]) @ np.abs(Rs[h].T))
            dt = 16 * EPS64 * (np.abs(t[tg]) + np.abs(R) @ np.abs(t[h]))
            p = pr[h * nF + tg]
            assert np.all(np.abs(p["RTll"].reshape(3, 3) - R) <= 8 * EPS * np.abs(R) + dR), (h, tg)
            assert np.all(np.abs(p["tTll"] - tr) <= 8 * EPS * np.abs(tr) + dt), (h, tg)
            a = np.exp(aff[tg, 0] - aff[h, 0]) * float(expo[tg]) / float(expo[h])
            b = aff[tg, 1] - a * aff[h, 1]
            assert abs(p["aff"][0] - a) <= 8 * EPS * abs(a), (h, tg)
            assert abs(p["aff"][1] - b) <= 8 * EPS * (abs(aff[tg, 1]) + abs(a * aff[h, 1])), (h, tg)
            if tg == new:
                ref = K1d @ R @ Kid
                bound = 8 * EPS * (np.abs(K1d) @ np.abs(R) @ np.abs(Kid)) + np.abs(K1d) @ dR @ np.abs(Kid)
                assert np.all(np.abs(fr[h]["KRKi"].reshape(3, 3) - ref) <= bound), h
                bound = 8 * EPS * (np.abs(K1d) @ np.abs(tr)) + np.abs(K1d) @ dt
                assert np.all(np.abs(fr[h]["Kt"] - K1d @ tr) <= bound), h


def mirror(nF, host, masks):
    from hslam_amd import _lib
    h = np.ascontiguousarray(host, np.int32)
    m = np.ascontiguousarray(masks, np.uint8)
    a, b = np.zeros((len(h), 12), np.int32), np.zeros((len(h), 12), np.int32)
    rc = _lib.load().hs_debug_act_mirror(nF, len(h), _lib.ptr(h), _lib.ptr(m), _lib.ptr(a), _lib.ptr(b))
    return rc, a, b


@pytest.mark.parametrize("nF", [2, 5, 8])
def test_mirror_rule_equals_insert_points_and_residuals(nF):
    """Hand-written hosts and IN masks: the residual order (ascending frame) and lastResiduals (an IN residual into
    the newest / second-newest frame: slot 0 / 1, else OOB without a frame) of the activation's mirror work equal
    hs_ba_insert_points + hs_ba_insert_residuals', and both the rule written out here."""
    host, masks = [], []
    for h in range(nF):
        for mk in range(1 << nF):
            if (mk >> h) & 1 or mk == 0 or bin(mk).count("1") > 7:
                continue
            host.append(h)
            masks.append(mk)
    host, masks = host[::3] + host[1::7], masks[::3] + masks[1::7]   # a few hundred points, hosts interleaved
    rc, a, b = mirror(nF, host, masks)
    assert rc == 0
    assert np.array_equal(a, b)
    for k, (h, mk) in enumerate(zip(host, masks)):
        tg = [t for t in range(nF) if (mk >> t) & 1]
        assert a[k, 0] == len(tg) and list(a[k, 1:1 + len(tg)]) == tg and np.all(a[k, 1 + len(tg):8] == -1)
        for s in range(2):
            t = nF - 1 - s
            has = t >= 0 and (mk >> t) & 1
            assert a[k, 8 + s] == (t if has else -1) and a[k, 10 + s] == (IN if has else OOB), (k, s)


def test_mirror_rule_rejects_a_residual_into_the_host_or_no_frame():
    assert mirror(4, [1], [0b0010])[0] != 0
    assert mirror(4, [1], [0b10001])[0] != 0
    assert mirror(4, [4], [0b0001])[0] != 0


@pytest.mark.parametrize("nF", [4, 8])
def test_scene_on_the_oracle(nF):
    """The window activation scene on the CPU oracle, its inputs formed on the host from the window's own poses:
    enough activated / deleted / kept points, on >= 3 hosts, with different residual counts."""
    from hslam_amd.scene import make_window_activation_scene
    from test_act import oracle_tracer
    bs, s = make_window_activation_scene(n_frames=nF)
    assert bs.n_points == 300 and len(s.imm_u) == 600 and (bs.width, bs.height) == (320, 240)
    aff = np.stack([bs.frames_state[:, 6] * 10.0, bs.frames_state[:, 7] * 1000.0], 1)
    fr, pr, _, _ = formed_inputs(bs.frames_eval, aff, bs.frames_exposure, s.K4)
    fr["slot"], fr["flagged_for_marg"] = s.slots, s.flagged
    assert np.array_equal(pr["aff"], s.aff)
    r = oracle_tracer(s).activatePointsMT(s.imgs, s.K4, fr, pr, s.act_frame, s.act_u, s.act_v, s.act_idepth,
                                          bs.n_points, 2.0, s.order)
    a = r["activated"]
    assert len(a) >= 20 and (r["action"] == 1).sum() >= 20 and (r["action"] == 0).sum() >= 20
    assert len(np.unique(s.imm_frame[a])) >= 3
    assert len({bin(int(x)).count("1") for x in r["res_in"][a]}) >= 2
