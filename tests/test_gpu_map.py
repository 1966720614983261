"""The point map (include/hs_map.h): the records a window's removals leave, KFDisplay::RefreshPC over them and
hs_ba_flag_frames_for_marginalization.

Everything here is exact.  A record is a copy of the window's device state, so it is compared bit for bit with the
read-backs taken through the existing API just before the point left.  The display cloud is compared bit for bit with
tests/map_ref.py (np.float32 operations in the reference's order) evaluated on those records and read-backs.  The frame
decision is categorical and compared with tests/map_ref.py's rule on hs_ba_get_frames read-backs.  Shapes as
tests/test_gpu_flag.py: 320x240, 10 keyframes, window 6, 80 points per keyframe."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_ref  # noqa: E402

pytestmark = pytest.mark.gpu

K_SMALL = np.array([[128.0, 0, 159.5], [0, 127.2, 119.5], [0, 0, 1.0]])
OUTLIER, MARGINALIZED = 1, 3
STATE_FIELDS = (("idepth", "idepth"), ("idepth_zero", "idepth_zero"), ("maxRelBaseline", "maxRelBaseline"),
                ("numGoodResiduals", "numGoodResiduals"), ("hdif", "HdiF"))


@pytest.fixture(scope="module")
def seq10():
    from hslam_amd.keyframe import make_ba_sequence
    return make_ba_sequence(n_kf=10, points_per_kf=80, seed=7, width=320, height=240, K=K_SMALL)


def hip():
    """The HIP runtime the product library has already loaded into this process."""
    with open("/proc/self/maps") as maps:
        path = next(line.split()[-1] for line in maps if "libamdhip64" in line)
    lib = C.CDLL(path)
    lib.hipMemcpy.argtypes, lib.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    return lib


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_records(recs, seq, cand_of, st, ps, pos, status, frames):
    """recs: the records of the points at window positions `pos` (in that order) of the window read back as st / ps."""
    assert len(recs) == len(pos)
    assert np.array_equal(recs["handle"], st["handles"][pos])
    assert np.array_equal(recs["status"], status)
    assert np.array_equal(recs["frame_id"], np.asarray(frames)[st["pt_host"][pos]])
    for rk, pk in STATE_FIELDS:
        assert _same(recs[rk], ps[pk][pos]), rk
    src = [cand_of[int(h)] for h in recs["handle"]]
    assert _same(recs["u"], np.array([seq.cand[k]["u"][i] for k, i in src], np.float32))
    assert _same(recs["v"], np.array([seq.cand[k]["v"][i] for k, i in src], np.float32))
    col = np.array([seq.cand[k]["color"][i] for k, i in src], np.float32).reshape(-1, 8)
    assert np.array_equal(recs["color"], map_ref.color_u8(col))
    assert not recs["reserved"].any()


def _want_cloud(drv, m, fid, kinv):
    """tests/map_ref.py on the frame's active points (read-backs) and its MARGINALIZED records."""
    ba, seq = drv.ba, drv.seq
    active = None
    if fid in drv.frames:
        st, ps = ba.structure(), ba.point_state()
        sel = st["pt_host"] == drv.frames.index(fid)
        src = [drv.cand_of[int(h)] for h in st["handles"][sel]]
        active = dict(u=np.array([seq.cand[k]["u"][i] for k, i in src], np.float32),
                      v=np.array([seq.cand[k]["v"][i] for k, i in src], np.float32), idepth=ps["idepth"][sel],
                      hdif=ps["HdiF"][sel], maxRelBaseline=ps["maxRelBaseline"][sel])
    recs = m.records()
    r = recs[(recs["frame_id"] == fid) & (recs["status"] == MARGINALIZED)]
    return map_ref.refresh_pc(active, dict(u=r["u"], v=r["v"], idepth=r["idepth"], hdif=r["hdif"],
                                           maxRelBaseline=r["maxRelBaseline"], color=r["color"]), kinv), active, r


def _check_cloud(drv, m, fid, cover=None):
    got = m.refresh_cloud(fid, drv.ba)
    (xyz, rgb), active, r = _want_cloud(drv, m, fid, got["kinv"])
    assert got["n"] == len(xyz) and got["n"] % 8 == 0, (fid, got["n"], len(xyz))
    assert _same(got["xyz"], xyz), fid
    assert _same(got["rgb"], rgb), fid
    if cover is not None:
        cover["kept"] += got["n"] // 8
        cover["empty"] += int(got["n"] == 0)
        cover["active"] += int(active is not None and got["n"] > 0 and (got["rgb"][0] == (0, 0, 255)).all())
        cover["records"] += int(len(r) > 0)
        cover["gone"] += int(active is None)
    return got


def test_kinv_and_refresh_properties(seq10):
    """kinv_out, repeatability, the device buffers, and a frame without a kept point, on the first window."""
    from hslam_amd.keyframe import KeyframeBA
    from hslam_amd.map import PointMap
    m = PointMap.create(1024)
    drv = KeyframeBA(seq10, window=6, decisions="device", map=m)
    drv.bootstrap()
    drv.add_keyframe(5)
    clouds = {f: _check_cloud(drv, m, f) for f in [0] + drv.frames}
    fid = max(clouds, key=lambda f: clouds[f]["n"] if f in drv.frames else -1)  # the fullest frame of the window
    a = clouds[fid]
    b = m.refresh_cloud(fid, drv.ba)
    assert a["n"] > 0 and a["n"] == b["n"] and _same(a["xyz"], b["xyz"]) and _same(a["rgb"], b["rgb"])
    # kinv_out: within 1 ulp of 1/fx, 1/fy, -cx/fx, -cy/fy in fp32, for the window's current calibration
    cal = drv.ba.frames()["calib"]  # CalibData::value: the scaled values / 50
    fx, fy, cx, cy = (np.float32(50.0 * v) for v in cal)
    want = np.array([np.float32(1) / fx, np.float32(1) / fy, -cx / fx, -cy / fy], np.float32)
    ulp = np.spacing(np.abs(want))
    assert (np.abs(a["kinv"].astype(np.float64) - want.astype(np.float64)) <= ulp).all(), (a["kinv"], want)
    assert abs(fx - 128.0) < 1.0 and abs(cy - 119.5) < 1.0
    # the device buffers hold what the host copies hold
    dx, dr, n = m.cloud_device()
    assert n == b["n"] and dx and dr
    hx, hr = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.uint8)
    rt = hip()
    assert rt.hipMemcpy(hx.ctypes.data, dx, hx.nbytes, 2) == 0 and rt.hipMemcpy(hr.ctypes.data, dr, hr.nbytes, 2) == 0
    assert _same(hx, b["xyz"]) and _same(hr, b["rgb"])
    # a smaller host capacity truncates the copy, not the count
    t = m.refresh_cloud(fid, drv.ba, cap=8)
    assert t["n"] == b["n"] and _same(t["xyz"], b["xyz"][:8])
    # a keyframe the map has never seen and the window does not hold: count 0, HS_OK; the newest keyframe hosts no
    # point yet (its candidates activate with the next keyframe): count 0 as well
    for f in (12345, drv.frames[-1]):
        e = m.refresh_cloud(f, drv.ba)
        assert e["n"] == 0 and e["xyz"].shape == (0, 3)
    # a keyframe that has left the window: its marginalized records alone
    assert 0 not in drv.frames and not (clouds[0]["rgb"] == (0, 0, 255)).all(1).any()
    assert m.lib.hs_map_refresh_cloud(m.h, None, 0, None, None, 0, None, None) == -1  # the calibration is the window's
    drv.ba.close()
    m.close()


@pytest.mark.parametrize("ppk", [80, 300])
def test_records_and_cloud_over_the_sequence(ppk, seq10):
    """KeyframeBA(decisions='device', map=...) over keyframes 5-9.  The records flagPointsForRemoval leaves are the
    action != 0 points in window order, every field equal to the read-backs taken at the 'marginalize' hook; the
    records removeOutliers leaves likewise.  After every keyframe the cloud of every frame id seen so far equals
    tests/map_ref.py.  300 points per keyframe: a frame's points cross the cloud kernel's 128-point chunks."""
    from hslam_amd.keyframe import KeyframeBA, make_ba_sequence
    from hslam_amd.map import PointMap
    seq = seq10 if ppk == 80 else make_ba_sequence(n_kf=10, points_per_kf=300, seed=7, width=320, height=240,
                                                   K=K_SMALL)
    m = PointMap.create(ppk * 12)
    drv = KeyframeBA(seq, window=6, decisions="device", map=m)
    drv.bootstrap()
    box, cover = {}, dict(kept=0, empty=0, active=0, records=0, gone=0, outliers_removed=0, chunk=0)

    def check(d, phase):
        if phase == "tail":  # before the drops and removeOutliers
            box["n_tail"] = len(m)
        elif phase == "marginalize":  # after removeOutliers, before flagPointsForRemoval
            box.update(st=d.ba.structure(), ps=d.ba.point_state(), frames=list(d.frames), n0=len(m),
                       cand_of=dict(d.cand_of))

    seen_ids = set(drv.frames)
    for k in range(5, 10):
        drv.add_keyframe(k, check=check)
        seen_ids |= set(drv.frames)
        act = drv.last_flags["action"]
        pos = np.nonzero(act)[0]
        recs = m.records(box["n0"])
        _check_records(recs, seq, box["cand_of"], box["st"], box["ps"], pos,
                       np.where(act[pos] == 2, MARGINALIZED, OUTLIER), box["frames"])
        assert set(recs["status"].tolist()) == {OUTLIER, MARGINALIZED}, k  # both occur at every keyframe
        # removeOutliers' records: OUTLIER, as many as it removed
        ro = m.records(box["n_tail"], box["n0"] - box["n_tail"])
        assert len(ro) == drv.history[-1]["dropped_points"] and (ro["status"] == OUTLIER).all()
        cover["outliers_removed"] += len(ro)
        # the host-side counters are the records' counts
        allr = m.records()
        for fid in seen_ids:
            sel = allr["frame_id"] == fid
            assert m.frame_counts(fid) == (int((sel & (allr["status"] == MARGINALIZED)).sum()),
                                           int((sel & (allr["status"] == OUTLIER)).sum()))
        assert m.size() == (len(allr), len(set(allr["frame_id"].tolist())))
        for fid in sorted(seen_ids):
            g = _check_cloud(drv, m, fid, cover)
            cover["chunk"] += int(g["n"] // 8 > 128)
    print(f"ppk {ppk}: records {len(m)}, cloud coverage {cover}")
    assert cover["kept"] > 0 and cover["active"] > 0 and cover["records"] > 0 and cover["gone"] > 0
    if ppk == 300:
        assert cover["chunk"] > 0
    drv.ba.close()
    m.close()


def test_attaching_a_map_changes_nothing(seq10):
    """The same sequence with and without a map: handle sets, HM / bM, frame states, energies and the final point
    state are bit-identical."""
    from hslam_amd.keyframe import KeyframeBA
    from hslam_amd.map import PointMap

    def run(with_map):
        m = PointMap.create(2048) if with_map else None
        drv = KeyframeBA(seq10, window=6, decisions="device", map=m)
        drv.bootstrap()
        out, box = [], {}

        def check(d, phase):
            if phase == "points_marginalized":
                box["pm"] = d.ba.marginal_prior()
            elif phase == "frame_marginalized":
                box["fm"] = d.ba.marginal_prior()

        for k in range(5, 10):
            info = drv.add_keyframe(k, check=check)
            out.append(dict(marg=drv.marg_handles.copy(), drop=drv.drop_handles.copy(), pm=box["pm"], fm=box["fm"],
                            frames=drv.ba.frames(), energies=np.asarray(info["energies"]),
                            gone=info["dropped_points"]))
        final = dict(structure=drv.ba.structure(), point_state=drv.ba.point_state(), last=drv.ba.lastResiduals())
        n = len(m) if with_map else 0
        drv.ba.close()
        if with_map:
            m.close()
        return out, final, n

    a, fa, n = run(True)
    b, fb, _ = run(False)
    assert n > 0
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x["marg"], y["marg"]) and np.array_equal(x["drop"], y["drop"]) and x["gone"] == y["gone"]
        for key in ("pm", "fm"):
            for p, q in zip(x[key], y[key]):
                assert _same(p, q), (k, key)
        for key in x["frames"]:
            assert _same(x["frames"][key], y["frames"][key]), (k, key)
        assert _same(x["energies"], y["energies"]), k
    for grp in fa:
        for key in fa[grp]:
            assert _same(fa[grp][key], fb[grp][key]), (grp, key)


def _planted(seq, m, n_frames=6):
    """The first window (no tail has run: every maxRelBaseline is what it was inserted with) plus planted points on the
    newest frame, then one GN iteration, so that HdiF is the solve's."""
    from hslam_amd.keyframe import KeyframeBA, in_bounds_targets
    drv = KeyframeBA(seq, window=8, decisions="device", map=m)
    drv.bootstrap(n_frames)
    ba, host = drv.ba, n_frames - 1
    c = seq.cand[host]
    n = len(c["u"])
    i = np.arange(n)
    # idepth < 0 for every 8th; the others at their depth; every other group of 8 with a maxRelBaseline under the 0.1
    # bar (no tail runs here, so the value stays as inserted)
    idepth = np.where(i % 8 == 7, -np.abs(c["idepth"]), c["idepth"]).astype(np.float32)
    rel = np.where((i // 8) % 2 == 0, 0.5, 0.05).astype(np.float32)
    hd = ba.insertPoints(np.full(n, host, np.int32), c["u"], c["v"], idepth, idepth, c["color"], c["weights"],
                         max_rel_baseline=rel, num_good=np.full(n, 5, np.int32))
    ok = in_bounds_targets(seq, host, drv.frames, c["u"], c["v"], np.abs(c["idepth"]))
    ok[(i % 8 == 3) | (i % 8 == 4)] = False  # no residual at all: nothing constrains the depth (var over its bar)
    pi, ti = np.nonzero(ok)
    ba.insertResiduals(hd[pi], ti.astype(np.int32))
    for j, h in enumerate(hd):
        drv.cand_of[int(h)] = (host, j)
    ba.makeIDX()
    ba.optimize(1)
    return drv, hd


def test_remove_outliers_retire_points_and_the_cloud_filters(seq10):
    """Planted points on the newest frame: removeOutliers' and hs_map_retire_points' records against read-backs taken
    just before; a bad handle and a bad status; then the cloud of that frame (active points and planted records) with
    a record on each side of each of RefreshPC's filters and one with idepth < 0."""
    from hslam_amd import _lib
    from hslam_amd.map import PointMap
    m = PointMap.create(2048)
    drv, hd = _planted(seq10, m)
    ba, lib, seq = drv.ba, _lib.load(), seq10
    host = len(drv.frames) - 1
    # ---- hs_map_retire_points: the odd planted points, mixed statuses, in an order of our own
    st, ps = ba.structure(), ba.point_state()
    mine = hd[1::2][::-1].copy()
    status = np.where(np.arange(len(mine)) % 5 == 4, OUTLIER, MARGINALIZED).astype(np.uint8)
    n1 = len(m)
    assert n1 == 0

    def retire(handles, stat):
        h, s = np.ascontiguousarray(handles, np.int32), np.ascontiguousarray(stat, np.uint8)
        return lib.hs_map_retire_points(ba.h, len(h), _lib.ptr(h), _lib.ptr(s))

    assert retire([int(mine[0]), 10 ** 6], [MARGINALIZED, MARGINALIZED]) == -1 and len(m) == n1   # unknown handle
    assert retire([int(mine[0]), -1], [MARGINALIZED, MARGINALIZED]) == -1 and len(m) == n1
    assert retire([int(mine[0]), int(mine[0])], [OUTLIER, OUTLIER]) == -1 and len(m) == n1         # listed twice
    for bad in (0, 2, 4):
        assert retire(mine[:2], [MARGINALIZED, bad]) == -1 and len(m) == n1                        # HS_ERR_INVALID
    assert retire(mine, status) == 0
    pos = np.array([int(np.nonzero(st["handles"] == h)[0][0]) for h in mine])
    recs = m.records(n1)
    _check_records(recs, seq, drv.cand_of, st, ps, pos, status, drv.frames)
    ba.removePoints(mine)
    ba.makeIDX()
    assert retire([int(mine[0])], [OUTLIER]) == -1 and len(m) == n1 + len(mine)                    # it has left
    counts = (int((status == MARGINALIZED).sum()), int((status == OUTLIER).sum()))
    assert m.frame_counts(drv.frames[host]) == counts
    # ---- removeOutliers: the even planted points without a residual, in its removal order
    st, ps = ba.structure(), ba.point_state()
    n0 = len(m)
    gone = ba.removeOutliers()
    want = st["handles"][st["nres"] == 0]
    assert len(gone) >= 8 and sorted(gone) == sorted(want) and np.isin(gone, hd).all()
    pos = np.array([int(np.nonzero(st["handles"] == h)[0][0]) for h in gone])
    _check_records(m.records(n0), seq, drv.cand_of, st, ps, pos, np.full(len(gone), OUTLIER), drv.frames)
    assert m.frame_counts(drv.frames[host]) == (counts[0], counts[1] + len(gone))
    # ---- removeOutliers of points inserted since the last commit: the call commits first, the records hold what was
    # inserted (no solve has seen them: HdiF 0)
    c5 = seq.cand[drv.frames[host]]
    n2 = len(m)
    new = ba.insertPoints(np.full(3, host, np.int32), c5["u"][:3], c5["v"][:3], c5["idepth"][:3], c5["idepth"][:3],
                          c5["color"][:3], c5["weights"][:3], max_rel_baseline=np.full(3, 0.25, np.float32),
                          num_good=np.full(3, 7, np.int32))
    gone2 = ba.removeOutliers()  # removal order: a removed entry takes the list's last one
    assert sorted(gone2) == sorted(new)
    j = np.array([int(np.nonzero(new == h)[0][0]) for h in gone2])
    r3 = m.records(n2)
    assert np.array_equal(r3["handle"], gone2) and (r3["status"] == OUTLIER).all()
    assert (r3["frame_id"] == drv.frames[host]).all() and _same(r3["idepth"], c5["idepth"][j])
    assert _same(r3["u"], c5["u"][j]) and (r3["maxRelBaseline"] == np.float32(0.25)).all()
    assert (r3["numGoodResiduals"] == 7).all() and (r3["hdif"] == 0).all()
    assert np.array_equal(r3["color"], map_ref.color_u8(c5["color"][j]))
    # ---- the cloud of the planted frame: the other half still active, the MARGINALIZED records behind them
    ba.makeIDX()
    got = _check_cloud(drv, m, drv.frames[host])
    r = recs[recs["status"] == MARGINALIZED]
    keep, _, term = map_ref.cloud_keep(r["idepth"], r["hdif"], r["maxRelBaseline"])
    pos_d = ~term["neg"]
    cover = {
        "idepth < 0": int(term["neg"].sum()),
        "kept": int(keep.sum()),
        "var * depth4 over": int((pos_d & term["scaled"] & ~term["absv"]).sum()),
        "var * depth4 under": int((pos_d & ~term["scaled"]).sum()),
        "var over": int((pos_d & term["absv"]).sum()),
        "var under": int((pos_d & ~term["absv"]).sum()),
        "maxRelBaseline under": int((pos_d & ~term["scaled"] & ~term["absv"] & term["base"]).sum()),
        "maxRelBaseline over": int((pos_d & ~term["scaled"] & ~term["absv"] & ~term["base"]).sum()),
    }
    print("planted records on each side of the filters:", cover, "vertices", got["n"])
    assert all(v > 0 for v in cover.values()), cover
    assert got["n"] > 0 and (got["rgb"][0] == (0, 0, 255)).all() and (got["rgb"][-1, 0] == got["rgb"][-1]).all()
    ba.close()
    m.close()


def test_capacity(seq10):
    """A map smaller than the first retire: HS_ERR_NOMEM, and neither the window nor the map has changed."""
    from hslam_amd import _lib
    from hslam_amd.keyframe import KeyframeBA
    from hslam_amd.map import PointMap
    lib = _lib.load()
    drv = KeyframeBA(seq10, window=6, decisions="device")
    drv.bootstrap()
    drv.add_keyframe(5, marginalize=False)
    m = PointMap.create(4)
    drv.ba.attachMap(m)
    ba = drv.ba
    st0, ps0, prior0 = ba.structure(), ba.point_state(), ba.marginal_prior()
    mf = np.zeros(1, np.int32)
    dry = ba.flagPointsForRemoval([0], apply=False)
    assert dry["counts"]["n_drop"] + dry["counts"]["n_marg"] > 4 and dry["counts"]["n_marg"] > 0
    assert lib.hs_ba_flag_points_for_removal(ba.h, 1, _lib.ptr(mf), 1, None, None, None, None) == -6  # HS_ERR_NOMEM
    assert b"capacity" in lib.hs_last_error()
    st1, ps1, prior1 = ba.structure(), ba.point_state(), ba.marginal_prior()
    for a, b in ((st0, st1), (ps0, ps1)):
        for key in a:
            assert _same(a[key], b[key]), key
    assert _same(prior0[0], prior1[0]) and _same(prior0[1], prior1[1])
    assert m.size() == (0, 0)
    # hs_map_retire_points likewise
    h = np.ascontiguousarray(st0["handles"][:5], np.int32)
    s = np.full(5, OUTLIER, np.uint8)
    assert lib.hs_map_retire_points(ba.h, 5, _lib.ptr(h), _lib.ptr(s)) == -6 and m.size() == (0, 0)
    assert lib.hs_map_retire_points(ba.h, 4, _lib.ptr(h), _lib.ptr(s)) == 0 and m.size() == (4, 1)
    m.clear()
    assert m.size() == (0, 0) and m.frame_counts(int(drv.frames[0])) == (0, 0)
    ba.close()
    m.close()


def _numpy_frame_flags(ba, m, frame_ids, exposures, kf_id, n_immature, P):
    """tests/map_ref.py's rule on hs_ba_get_frames read-backs, the map's counters and the caller's inputs."""
    from hslam_amd.scene import se3_from_data
    fr, st = ba.frames(), ba.structure()
    nF = len(frame_ids)
    Rt = [se3_from_data(p) for p in fr["pose"]]  # PRE_worldToCam
    dist = np.zeros((nF, nF), np.float32)
    for h in range(nF):
        Rh, th = Rt[h]
        for t in range(nF):
            R, tt = Rt[t]
            dist[h, t] = np.float32(np.linalg.norm(tt - R @ (Rh.T @ th)))
    a = fr["state"][:, 6] * 10.0  # aff_g2l().a = state_scaled[6] = SCALE_A * state[6]
    aff0 = np.array([map_ref.affine_factor(exposures[-1], exposures[f], a[-1], a[f]) for f in range(nF)])
    n_in = np.array([(st["pt_host"] == f).sum() for f in range(nF)], np.int32) + np.asarray(n_immature, np.int32)
    n_out = np.array([sum(m.frame_counts(int(fid))) for fid in frame_ids], np.int32)
    flags, why = map_ref.frame_rule(n_in, n_out, aff0, dist, np.asarray(kf_id), P)
    return flags, why, dict(n_in=n_in, n_out=n_out, aff0=aff0, dist=dist)


def test_frame_decision_over_the_sequence(seq10):
    """frame_policy='reference': at every keyframe the library's flags equal the numpy rule on the read-backs."""
    from hslam_amd.keyframe import KeyframeBA
    from hslam_amd.map import PointMap
    m = PointMap.create(2048)
    drv = KeyframeBA(seq10, window=6, decisions="device", map=m, frame_policy="reference")
    drv.bootstrap()
    box, picks = {}, []

    def check(d, phase):
        if phase == "flag_frames":
            box["want"] = _numpy_frame_flags(d.ba, m, d.frames, [1.0] * len(d.frames), d.frame_inputs["kf_id"],
                                             d.frame_inputs["n_immature"], d.frame_params)

    for k in range(5, 10):
        info = drv.add_keyframe(k, check=check)
        want, why, inp = box["want"]
        assert np.array_equal(drv.frame_flags, want), (k, drv.frame_flags, want, inp)
        assert info["marg_frames"] == np.nonzero(want)[0].tolist() and len(info["marg_frames"]) == 1
        assert why[info["marg_frames"][0]] == map_ref.WHY_SCORE and len(drv.frames) == 5
        picks.append(info["marg_frames"][0])
    print("marginalized window frames per keyframe:", picks)
    assert picks[0] != 0  # KfId 0 is never the score's pick while it is in the window
    drv.ba.close()
    m.close()


def test_frame_decision_planted_window_and_errors(seq10):
    """Seven keyframes, one with a long exposure, one that has lost all but two of its points to the map: the affine
    rule, the 5 % rule and the distance score each flag a frame of their own.  Without a map: HS_ERR_STATE."""
    from hslam_amd import _lib
    from hslam_amd.ba import make_frame
    from hslam_amd.keyframe import KeyframeBA
    from hslam_amd.map import PointMap, frame_marg_params
    lib = _lib.load()
    expo = [1.0, 1.0, float(np.exp(0.9)), 1.0, 1.0, 1.0, 1.0]  # |log| = 0.9: 0.2 over the bar
    m = PointMap.create(1024)
    drv = KeyframeBA(seq10, window=8, decisions="device", map=m)
    drv._frame = lambda k: make_frame(seq10.evals[k], exposure=expo[k], energyTH=8 * 8 * 8, fid=k)
    drv.bootstrap(7)
    ba = drv.ba
    st = ba.structure()
    mine = st["handles"][st["pt_host"] == 3]
    ba.retirePoints(mine[2:], np.full(len(mine) - 2, MARGINALIZED, np.uint8))  # 2 stay: 2 < 0.05 * n for n > 40
    ba.removePoints(mine[2:])
    assert len(mine) >= 60 and m.frame_counts(3) == (len(mine) - 2, 0)
    kf_id = np.arange(7, dtype=np.int32) + 3
    n_imm = np.array([0, 0, 0, 0, 0, 0, 80], np.int32)
    P = frame_marg_params(maxFrames=5, minFrames=3)
    want, why, inp = _numpy_frame_flags(ba, m, drv.frames, expo, kf_id, n_imm, P)
    got = ba.flagFramesForMarginalization(kf_id, n_imm, P)
    print("planted window: flags", got, "why", why, "in", inp["n_in"], "out", inp["n_out"],
          "log aff", np.log(inp["aff0"]))
    assert np.array_equal(got, want)
    assert why[3] == map_ref.WHY_POINTS and why[2] == map_ref.WHY_AFFINE
    pick = np.nonzero(why == map_ref.WHY_SCORE)[0]
    assert len(pick) == 1 and got.sum() == 3
    sc = sorted(s for s in map_ref.frame_scores(inp["dist"], kf_id, P.minFrameAge) if s is not None)
    assert sc[1] - sc[0] >= 1e-3 * abs(sc[0]), sc[:2]
    # the reference's settings on the same window: 7 - 2 < maxFrames, so only the two clauses flag
    got = ba.flagFramesForMarginalization(kf_id, n_imm)
    want, why, _ = _numpy_frame_flags(ba, m, drv.frames, expo, kf_id, n_imm, frame_marg_params())
    assert np.array_equal(got, want) and got.tolist() == [0, 0, 1, 1, 0, 0, 0]
    # without a map: HS_ERR_STATE
    ba.attachMap(None)
    out = np.zeros(7, np.uint8)
    assert lib.hs_ba_flag_frames_for_marginalization(ba.h, None, _lib.ptr(kf_id), None, _lib.ptr(out), None) == -5
    assert b"map" in lib.hs_last_error()
    ba.close()
    m.close()


def test_lifetime_and_attach_errors(scene_small, seq10):
    from hslam_amd import _lib
    from hslam_amd.ba import BAWindow
    from hslam_amd.keyframe import KeyframeBA
    from hslam_amd.map import PointMap
    lib = _lib.load()
    lib.hs_debug_live_allocations.restype = C.c_longlong
    lib.hs_debug_live_allocations.argtypes = []
    live0 = lib.hs_debug_live_allocations()
    # create / attach / sequence / detach / destroy
    m = PointMap.create(1024)
    live_map = lib.hs_debug_live_allocations()
    assert live_map > live0
    drv = KeyframeBA(seq10, window=6, decisions="device", map=m)
    drv.bootstrap()
    drv.add_keyframe(5)
    live_run = lib.hs_debug_live_allocations()
    drv.add_keyframe(6)
    for fid in (0, 1, drv.frames[0]):
        m.refresh_cloud(fid, drv.ba)
    assert lib.hs_debug_live_allocations() == live_run  # nothing in the map path allocates
    n = len(m)
    assert n > 0
    other = PointMap.create(16)
    assert lib.hs_ba_attach_map(drv.ba.h, other.h) == -5   # the context has a map
    drv.ba.attachMap(None)
    drv.ba.attachMap(other)
    assert lib.hs_ba_attach_map(drv.ba.h, other.h) == 0    # attaching the same map again is a no-op
    drv.ba.attachMap(None)
    other.close()
    assert len(m) == n and len(m.records()) == n           # a detached map still reads
    drv.ba.close()
    m.close()
    assert lib.hs_debug_live_allocations() == live0
    # either may go first while attached
    for map_first in (True, False):
        m = PointMap.create(64)
        w = BAWindow(scene_small)
        w.attachMap(m)
        (m.close(), w.close()) if map_first else (w.close(), m.close())
        assert lib.hs_debug_live_allocations() == live0
    # a rank group refuses a map
    m = PointMap.create(64)
    grp = BAWindow.rank_group([scene_small.shard(r, 2) for r in range(2)])
    assert lib.hs_ba_attach_map(grp.members[0].h, m.h) == -5  # HS_ERR_STATE
    assert b"single-rank" in lib.hs_last_error()
    grp.close()
    m.close()
    assert lib.hs_debug_live_allocations() == live0
