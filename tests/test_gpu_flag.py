"""hs_ba_flag_points_for_removal: System::flagPointsForRemoval (Src/Mapping.cpp:248-328) decided on the device, and
the MapPoint::lastResiduals bookkeeping it needs (hs_ba_get_last_residuals / hs_ba_set_last_residuals).

The decisions are categorical, so every comparison here is exact: against the numpy rule applied to the library's own
read-backs (planted window), against the host-decided driver (bit for bit over a sequence), and against the CPU oracle
chain (the same point sets at every keyframe)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IN, OOB, OUT = 0, 1, 2
K_SMALL = np.array([[128.0, 0, 159.5], [0, 127.2, 119.5], [0, 0, 1.0]])


@pytest.fixture(scope="module")
def seq10():
    from hslam_amd.keyframe import make_ba_sequence
    return make_ba_sequence(n_kf=10, points_per_kf=80, seed=7, width=320, height=240, K=K_SMALL)


def _readbacks(ba):
    st, res, ps, lr = ba.structure(), ba.residuals(), ba.point_state(), ba.lastResiduals()
    return dict(handles=st["handles"], host=st["pt_host"], nres=st["nres"], res_point=st["res_point"],
                res_target=st["res_target"], res_state=res["state"], idepth=ps["idepth"],
                ngood=ps["numGoodResiduals"], hdif=ps["HdiF"], last0=lr["state"][:, 0].astype(int),
                last1=lr["state"][:, 1].astype(int))


def _rule(rb, marg_frames):
    """flagPointsForRemoval in numpy on the read-backs: masks of every clause, the actions and the six counters."""
    mf = np.asarray(marg_frames, int)
    n = len(rb["handles"])
    vis = np.zeros(n, int)
    sel = np.isin(rb["res_target"], mf) & (rb["res_state"] == IN)
    np.add.at(vis, rb["res_point"][sel], 1)
    nres, ng, l0, l1 = rb["nres"], rb["ngood"], rb["last0"], rb["last1"]
    drop_now = (rb["idepth"] < 0) | (nres == 0)
    vis_rule = (nres >= 3) & (ng > 14) & (nres - vis < 3)
    outout = (nres >= 2) & (l0 == OUT) & (l1 == OUT)
    oob = vis_rule | (l0 == OOB) | outout
    host_flagged = np.isin(rb["host"], mf)
    flag = (oob | host_flagged) & ~drop_now
    inl = (nres >= 3) & (ng >= 4)
    h = rb["hdif"].astype(np.float64)
    with np.errstate(divide="ignore"):
        hi = np.where(h > 0, 1.0 / h, 0.0) > 50.0
    action = np.zeros(n, np.uint8)
    action[drop_now | (flag & ~(inl & hi))] = 1
    action[flag & inl & hi] = 2
    counts = dict(flag_nores=int(drop_now.sum()), flag_oob=int(flag.sum()), flag_in=int((flag & inl).sum()),
                  flag_inin=int((flag & inl & hi).sum()), n_drop=int((action == 1).sum()),
                  n_marg=int((action == 2).sum()))
    return dict(action=action, counts=counts, vis=vis, drop_now=drop_now, vis_rule=vis_rule, outout=outout, oob=oob,
                host_flagged=host_flagged, flag=flag, inl=inl, hi=hi)


# the planted points (hosted by the newest frame 5; the frame to marginalize is 0):
# (residual targets, their states, numGoodResiduals seed, idepth sign, lastResiduals states)
PLANTED = [
    ([3, 4], [IN, IN], 5, -1, (IN, IN)),                # idepth < 0
    ([], [], 5, 1, (IN, IN)),                           # nres == 0
    ([0, 3, 4], [IN, IN, IN], 15, 1, (IN, IN)),         # the vis rule: 3 residuals, one IN into the marg frame
    ([0, 4], [IN, IN], 15, 1, (IN, IN)),                # ... blocked by nres < 3
    ([0, 3, 4], [IN, IN, IN], 14, 1, (IN, IN)),         # ... blocked by numGoodResiduals <= 14
    ([0, 2, 3, 4], [IN, IN, IN, IN], 15, 1, (IN, IN)),  # ... blocked by nres - vis >= 3
    ([0, 3, 4], [OUT, IN, IN], 15, 1, (IN, IN)),        # ... blocked: the residual into the marg frame is not IN
    ([3, 4], [IN, IN], 5, 1, (OOB, IN)),                # last0 == OOB; not an inlier by nres
    ([3, 4], [IN, IN], 5, 1, (OUT, OUT)),               # OUT / OUT
    ([4], [IN], 5, 1, (OUT, OUT)),                      # OUT / OUT blocked by nres < 2
    ([2, 3, 4], [IN, IN, IN], 3, 1, (OOB, IN)),         # flagged, not an inlier by numGoodResiduals
    ([2, 3, 4], [IN, IN, IN], 4, 1, (OOB, OUT)),        # a flagged inlier
    ([2, 3, 4], [IN, OUT, IN], 4, 1, (OUT, IN)),        # OUT / IN: kept
    ([1, 2, 3, 4], [IN, IN, IN, IN], 20, 1, (IN, OUT)),  # kept
]


def test_planted_window_dry_run_and_apply():
    from hslam_amd.keyframe import KeyframeBA, make_ba_sequence
    seq = make_ba_sequence(n_kf=6, points_per_kf=40, width=320, height=240, K=K_SMALL)
    drv = KeyframeBA(seq, window=8)
    drv.bootstrap(6)
    ba = drv.ba
    c = seq.cand[5]
    n = min(40, len(c["u"]))
    case = np.arange(n) % len(PLANTED)
    sign = np.array([PLANTED[k][3] for k in case], np.float32)
    idepth = (np.abs(c["idepth"][:n]) * sign).astype(np.float32)
    hd = ba.insertPoints(np.full(n, 5, np.int32), c["u"][:n], c["v"][:n], idepth, idepth, c["color"][:n],
                         c["weights"][:n], num_good=np.array([PLANTED[k][2] for k in case], np.int32))
    rh = np.concatenate([np.full(len(PLANTED[k][0]), hd[i]) for i, k in enumerate(case)]).astype(np.int32)
    rt = np.concatenate([PLANTED[k][0] for k in case]).astype(np.int32)
    rs = np.concatenate([PLANTED[k][1] for k in case]).astype(np.uint8)
    ba.insertResiduals(rh, rt, rs)
    ba.setLastResiduals(hd, np.full((n, 2), -1, np.int32), np.array([PLANTED[k][4] for k in case], np.uint8))
    ba.makeIDX()

    # ---- before any solve: HdiF is 0 everywhere, every flagged inlier is dropped
    seen = {}
    for mf in ([0], [0, 5]):
        rb = _readbacks(ba)
        want = _rule(rb, mf)
        got = ba.flagPointsForRemoval(mf, apply=False)
        print(f"marg frames {mf}: counts {got['counts']}")
        assert np.array_equal(got["action"], want["action"])
        assert got["counts"] == want["counts"]
        assert not want["hi"].any() and got["counts"]["n_marg"] == 0 and got["counts"]["flag_in"] > 0
        seen[len(mf)] = want
    w = seen[1]
    planted = np.isin(_readbacks(ba)["handles"], hd)
    rb = _readbacks(ba)
    nres, ng, vis = rb["nres"], rb["ngood"], w["vis"]
    occurs = {
        "idepth < 0": rb["idepth"] < 0,
        "nres == 0": nres == 0,
        "vis rule": w["vis_rule"] & (nres == 3) & (ng == 15) & (vis == 1) & ~w["drop_now"],
        "vis rule blocked by nres": (nres < 3) & (ng > 14) & (nres - vis < 3) & (nres > 0),
        "vis rule blocked by nGood": (nres >= 3) & (ng <= 14) & (ng > 4) & (nres - vis < 3),
        "vis rule blocked by nres - vis": (nres >= 3) & (ng > 14) & (nres - vis >= 3) & planted,
        "last0 == OOB": (rb["last0"] == OOB) & ~w["drop_now"] & planted,
        "OUT/OUT": w["outout"] & ~w["drop_now"],
        "OUT/OUT blocked by nres": (nres < 2) & (nres > 0) & (rb["last0"] == OUT) & (rb["last1"] == OUT),
        "host flagged": w["host_flagged"] & ~w["oob"] & ~w["drop_now"],
        "inl false by nres": w["flag"] & (nres < 3) & (ng >= 4),
        "inl false by nGood": w["flag"] & (nres >= 3) & (ng < 4),
        "flagged inlier, hi false": w["flag"] & w["inl"] & ~w["hi"],
        "kept": w["action"] == 0,
    }
    for name, m in occurs.items():
        assert m.any(), name
    # the blocked cases are kept, the others leave
    for name in ("vis rule blocked by nres", "vis rule blocked by nGood", "vis rule blocked by nres - vis",
                 "OUT/OUT blocked by nres"):
        assert (w["action"][occurs[name] & planted] == 0).all(), name
    for name in ("idepth < 0", "nres == 0", "vis rule", "last0 == OOB", "OUT/OUT", "host flagged"):
        assert (w["action"][occurs[name]] == 1).all(), name
    # with two marg frames the planted points' host is flagged too
    assert seen[2]["host_flagged"][planted].all() and not seen[1]["host_flagged"][planted].any()
    # a dry run changed nothing
    assert np.array_equal(_readbacks(ba)["handles"], rb["handles"])

    # ---- apply before the solve: nothing is marginalized, HM / bM untouched, the flagged points leave
    HM0, bM0 = ba.marginal_prior()
    got = ba.flagPointsForRemoval([0], apply=True, return_prior=True)
    assert got["counts"]["n_marg"] == 0 and got["counts"]["n_drop"] > 0
    assert np.array_equal(got["action"], w["action"])
    HM1, bM1 = ba.marginal_prior()
    for a in (got["HM"], HM1):
        assert a.tobytes() == HM0.tobytes()
    for a in (got["bM"], bM1):
        assert a.tobytes() == bM0.tobytes()
    left = ba.structure()
    assert sorted(left["handles"]) == sorted(rb["handles"][w["action"] == 0])
    assert not (left["pt_host"] == 0).any()
    lr = ba.lastResiduals()["state"]  # the pairs followed their points through the commit
    pos = {int(h): i for i, h in enumerate(rb["handles"])}
    for i, h in enumerate(left["handles"]):
        assert lr[i, 0] == rb["last0"][pos[int(h)]] and lr[i, 1] == rb["last1"][pos[int(h)]]

    # ---- after a solve and the tail: HdiF is set, flagged inliers are marginalized
    ba.optimize(1)
    ba.fixLinearization(None, None, False)
    for mf in ([1], [1, 2]):
        rb = _readbacks(ba)
        want = _rule(rb, mf)
        got = ba.flagPointsForRemoval(mf, apply=False)
        print(f"after the solve, marg frames {mf}: counts {got['counts']}")
        assert np.array_equal(got["action"], want["action"])
        assert got["counts"] == want["counts"]
        assert got["counts"]["flag_inin"] > 0 and got["counts"]["n_marg"] == got["counts"]["flag_inin"]
    ba.close()


def _by_handle(ba):
    lr = ba.lastResiduals()
    return ba.structure()["handles"], lr


def test_last_residuals_follow_the_host_bookkeeping(seq10):
    """Host-decided driver: after every tail and every commit the device's lastResiduals states equal the driver's own
    bookkeeping (drv.last_state) for every handle."""
    from hslam_amd.keyframe import KeyframeBA
    drv = KeyframeBA(seq10, window=6)
    drv.bootstrap()
    seen = dict(checks=0, targets=0, states=set())

    def compare(d, nF):
        hd, lr = _by_handle(d.ba)
        want = np.array([d.last_state[int(h)] for h in hd], np.uint8).reshape(len(hd), 2)
        assert np.array_equal(lr["state"], want)
        t = lr["target"]
        assert np.isin(t[:, 0], (-1, nF - 1)).all() and np.isin(t[:, 1], (-1, nF - 2)).all()
        seen["checks"] += 1
        seen["targets"] += int((t >= 0).sum())
        seen["states"] |= set(np.unique(want).tolist())

    def check(d, phase):
        # 'optimize': the commit of the new frame, its residuals and the activated points; 'marginalize': after the
        # tail (the driver has taken the tail's states) and the commit of its drops; 'frame_marginalized': the commit
        # of the removed points and frame
        if phase in ("optimize", "marginalize", "frame_marginalized"):
            compare(d, len(d.frames))

    compare(drv, len(drv.frames))
    for k in range(5, 10):
        drv.add_keyframe(k, check=check)
        compare(drv, len(drv.frames))
    assert seen["checks"] == 1 + 5 * 4 and seen["targets"] > 0 and seen["states"] == {IN, OOB, OUT}
    drv.ba.close()


def test_device_decisions_equal_host_decisions(seq10):
    """Two drivers over the same sequence, decisions='host' and 'device': identical handle sets, HM / bM, frame states
    and point state at every keyframe, bit for bit."""
    from hslam_amd.keyframe import KeyframeBA
    logs, cover = {}, dict(last0_oob=0, outout=0, outout_blocked=0, flagged_not_inlier=0, host_flagged=0,
                           marginalized=0, dropped=0)

    def run(mode):
        drv = KeyframeBA(seq10, window=6, decisions=mode)
        drv.bootstrap()
        out = []
        box = {}

        def check(d, phase):
            if phase == "marginalize" and mode == "host":  # what the host path's own decisions cover
                st, ps = d.ba.structure(), d.ba.point_state()
                l0 = np.array([d.last_state[int(h)][0] for h in st["handles"]])
                l1 = np.array([d.last_state[int(h)][1] for h in st["handles"]])
                nres, ng = st["nres"], ps["numGoodResiduals"]
                flagged = np.isin(st["handles"], np.concatenate([d.marg_handles, d.drop_handles]))
                cover["last0_oob"] += int((l0 == OOB).sum())
                cover["outout"] += int(((nres >= 2) & (l0 == OUT) & (l1 == OUT)).sum())
                cover["outout_blocked"] += int(((nres < 2) & (l0 == OUT) & (l1 == OUT)).sum())
                cover["flagged_not_inlier"] += int((flagged & ~((nres >= 3) & (ng >= 4))).sum())
                cover["host_flagged"] += int((st["pt_host"] == d.marg_frame).sum())
                cover["marginalized"] += len(d.marg_handles)
                cover["dropped"] += len(d.drop_handles)
            elif phase == "points_marginalized":
                box["pm"] = d.ba.marginal_prior()
            elif phase == "frame_marginalized":
                box["fm"] = d.ba.marginal_prior()

        for k in range(5, 10):
            info = drv.add_keyframe(k, check=check)
            out.append(dict(marg=sorted(map(int, drv.marg_handles)), drop=sorted(map(int, drv.drop_handles)),
                            pm=box["pm"], fm=box["fm"], frames=drv.ba.frames(), energies=np.asarray(info["energies"]),
                            n=(info["marginalized_points"], info["dropped"])))
        final = dict(structure=drv.ba.structure(), point_state=drv.ba.point_state(), last=drv.ba.lastResiduals())
        drv.ba.close()
        return out, final

    logs["host"], fin_h = run("host")
    logs["device"], fin_d = run("device")
    print("host path coverage:", cover)
    assert all(v >= 1 for v in cover.values()), cover
    for k, (h, d) in enumerate(zip(logs["host"], logs["device"])):
        assert h["marg"] == d["marg"] and h["drop"] == d["drop"] and h["n"] == d["n"], k
        assert len(h["marg"]) > 0 and len(h["drop"]) > 0
        for key in ("pm", "fm"):
            for a, b in zip(h[key], d[key]):
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), (k, key)
        for key in h["frames"]:
            assert h["frames"][key].tobytes() == d["frames"][key].tobytes(), (k, key)
        assert h["energies"].tobytes() == d["energies"].tobytes(), k
    for grp in ("structure", "point_state", "last"):
        for key in fin_h[grp]:
            assert fin_h[grp][key].tobytes() == fin_d[grp][key].tobytes(), (grp, key)


def test_device_decisions_sequence_vs_oracle():
    """test_keyframe_sequence_drift_vs_oracle's configuration and bars (tests/test_gpu_window.py, measured there) with
    the decisions on the device: at every keyframe the oracle chain marginalizes and drops as many points, and the
    final point sets are identical."""
    from oracle_keyframe import OracleKeyframeBA
    from hslam_amd.keyframe import KeyframeBA, make_ba_sequence
    seq = make_ba_sequence(n_kf=12, points_per_kf=200, seed=7)
    drv = KeyframeBA(seq, window=8, image_path="raw", decisions="device")
    drv.bootstrap()
    orc = OracleKeyframeBA(seq, window=8)
    orc.bootstrap()
    for k in range(7, 12):
        ig = drv.add_keyframe(k)
        io = orc.add_keyframe(k)
        eg, eo = np.asarray(ig["energies"]), np.asarray(io["energies"])
        rel = np.abs(eg - eo) / np.abs(eo)
        print(f"kf {k}: energies rel dev max {rel.max():.2e}; marginalized gpu {ig['marginalized_points']} oracle "
              f"{io['marginalized_points']}; dropped gpu {ig['dropped']} oracle {io['dropped']}")
        assert ig["iters"] == io["iters"]
        assert rel.max() <= 3e-3, (k, rel)
        assert ig["marginalized_points"] == io["marginalized_points"] and ig["dropped"] == io["dropped"], k
        assert ig["marginalized_points"] > 0
    assert drv.frames == orc.frames
    fg, fo = drv.ba.frames(), orc.frame_states()
    fe = drv.ba.frame_eval()
    ds = np.abs(fg["state"] - fo["state"]).max()
    de = np.abs(fe["evalPT"] - fo["eval"]).max()
    dc = np.abs(fg["calib"] - fo["calib"]).max()
    HMg, bMg = drv.ba.marginal_prior()
    scale = np.abs(np.diag(orc.HM)).max()
    dH = (np.abs(HMg - orc.HM) / (np.abs(orc.HM) + 1e-3 * scale)).max()
    db = np.linalg.norm(bMg - orc.bM) / np.linalg.norm(orc.bM)
    pg = {drv.cand_of[int(h)]: float(d) for h, d in zip(drv.ba.structure()["handles"], drv.ba.point_state()["idepth"])}
    po = orc.point_idepth()
    common = sorted(set(pg) & set(po))
    dd = max(abs(pg[key] - po[key]) / abs(po[key]) for key in common)
    print(f"final: frame state |d| {ds:.2e}, evalPT |d| {de:.2e}, calib |d| {dc:.2e}, HM worst ratio {dH:.2e}, "
          f"bM rel norm {db:.2e}, points common {len(common)} differing {len(set(pg) ^ set(po))}, idepth rel {dd:.2e}")
    assert set(pg) == set(po)
    assert ds <= 2e-4 and de <= 2e-4 and dc <= 1e-8 and dH <= 3e-3 and db <= 3e-3 and dd <= 3e-4
    drv.ba.close()


def test_errors_and_lifetime(scene_small, seq10):
    from hslam_amd import _lib
    from hslam_amd.ba import BAWindow
    from hslam_amd.keyframe import KeyframeBA
    lib = _lib.load()
    lib.hs_debug_live_allocations.restype = C.c_longlong
    lib.hs_debug_live_allocations.argtypes = []
    live0 = lib.hs_debug_live_allocations()

    def call(ba, frames):
        mf = np.asarray(frames, np.int32)
        return lib.hs_ba_flag_points_for_removal(ba.h, len(mf), _lib.ptr(mf), 0, None, None, None, None)

    # create / reserve / sequence / destroy
    drv = KeyframeBA(seq10, window=6, decisions="device")
    drv.bootstrap()
    drv.add_keyframe(5)
    nF = len(drv.frames)
    assert call(drv.ba, [nF]) == -1 and call(drv.ba, [-1]) == -1 and call(drv.ba, [0, nF]) == -1  # HS_ERR_INVALID
    assert lib.hs_ba_flag_points_for_removal(drv.ba.h, 1, None, 0, None, None, None, None) == -1
    assert call(drv.ba, [0]) == 0 and call(drv.ba, []) == 0
    drv.ba.close()
    # a window set whole: lastResiduals derived from it; a rank group is refused
    full = BAWindow(scene_small)
    lr = full.lastResiduals()
    st = full.structure()
    nF = scene_small.n_frames
    has = np.zeros((len(st["handles"]), nF), bool)
    has[st["res_point"], st["res_target"]] = True
    assert np.array_equal(lr["target"][:, 0], np.where(has[:, nF - 1], nF - 1, -1))
    assert np.array_equal(lr["target"][:, 1], np.where(has[:, nF - 2], nF - 2, -1))
    assert np.array_equal(lr["state"][:, 0] == OOB, ~has[:, nF - 1])  # a fresh window's residuals are IN
    assert call(full, [0]) == 0
    full.close()
    grp = BAWindow.rank_group([scene_small.shard(r, 2) for r in range(2)])
    assert call(grp.members[0], [0]) == -5  # HS_ERR_STATE
    assert b"single-rank" in lib.hs_last_error()
    grp.close()
    assert lib.hs_debug_live_allocations() == live0
