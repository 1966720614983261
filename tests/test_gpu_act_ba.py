"""hs_tracer_activate_ba: System::activatePointsMT whose window is the BA context's, device to device -- the inputs
formed from the window on the device, the activated points staged into it on the device, the tracer compacted on the
device -- against the host path at the same commit: hs_tracer_activate fed the arrays hs_tracer_get_act_inputs
returns, then get_points, insertPoints, insertResiduals, compact.  Both run on fresh (BA window, tracer) pairs built
from one scene through the incremental API; every comparison is bit for bit.

Scene: make_window_activation_scene (300 active, 600 immature, 320 x 240, seed 7) at 4 and 8 frames (5 for the
pending-edits test).  The window holds the points of every frame but the newest, as at this point of AddKeyframe.
Every test asserts that the reference path activates, deletes and keeps >= 20 points, activates on >= 3 hosts and
gives points with different residual counts."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CMAD = 2.0


@functools.lru_cache(maxsize=None)
def scene(nF):
    from hslam_amd.scene import make_window_activation_scene
    return make_window_activation_scene(n_frames=nF)


def frame_of(bs, f):
    from hslam_amd.ba import make_frame
    return make_frame(bs.frames_eval[f], bs.frames_state[f], bs.frames_state_zero[f], bs.frames_exposure[f],
                      bs.frames_energyTH[f], bs.frames_id[f])


def build_window(bs, first=0, drop_first=False, capacity=2000):
    """AddKeyframe up to the activation: every frame but the newest committed with its points and the scene's
    residuals among them; then, uncommitted, (drop_first: frame `first`'s points removed and the frame dropped,)
    the newest frame inserted and hs_ba_add_residuals_to_newest.  Returns (ba, window frames as scene frames)."""
    from hslam_amd.ba import BAWindow
    nF = bs.n_frames
    ba = BAWindow(camera=(bs.width, bs.height, bs.n_levels, bs.K), capacity=capacity)
    old = list(range(first, nF - 1))
    for f in old:
        ba.insertFrame(frame_of(bs, f), image=bs.pyramids[f][0])
    sel = np.nonzero(np.isin(bs.pt_host, old))[0]
    win = {f: i for i, f in enumerate(old)}
    hd = ba.insertPoints([win[h] for h in bs.pt_host[sel]], bs.pt_u[sel], bs.pt_v[sel], bs.pt_idepth[sel],
                         bs.pt_idepth_zero[sel], bs.pt_color[sel], bs.pt_weights[sel])
    handle = -np.ones(bs.n_points, np.int64)
    handle[sel] = hd
    r = np.isin(bs.res_target, old) & (handle[bs.res_point] >= 0)
    ba.insertResiduals(handle[bs.res_point[r]], [win[t] for t in bs.res_target[r]])
    ba.makeIDX()
    frames = old
    if drop_first:
        ba.removePoints(hd[bs.pt_host[sel] == first])
        ba.removeFrame(0, marginalize=False)
        frames = old[1:]
    ba.insertFrame(frame_of(bs, nF - 1), image=bs.pyramids[nF - 1][0])
    ba.addResidualsToNewest()
    return ba, frames + [nF - 1]


def build_tracer(s, n_imm=None, quality=None):
    from hslam_amd.trace import ImmatureTracer
    n = len(s.imm_u) if n_imm is None else n_imm
    g = ImmatureTracer(s.width, s.height, max(1, n))
    for f in range(s.n_frames):
        g.set_host_image(int(s.slots[f]), s.imgs[f])
    if n:
        g.add_points(s.slots[s.imm_frame[:n]], s.imm_u[:n], s.imm_v[:n])
        g.set_state(s.imm_idepth_min[:n], s.imm_idepth_max[:n], s.imm_quality[:n] if quality is None else quality,
                    s.imm_status[:n], s.imm_interval[:n])
        g.set_types(s.imm_type[:n])
    return g


def drop_flags(s, frames):
    d = np.zeros(64, np.uint8)
    d[[int(s.slots[f]) for f in range(s.n_frames) if f not in frames]] = 1
    return d


def readbacks(ba):
    """Everything of the committed window the two paths have to agree on, then one linearizeAll and optimize(3)."""
    st, ps, res, lr = ba.structure(), ba.point_state(), ba.residuals(), ba.lastResiduals()
    o = {"st." + k: v for k, v in st.items()}
    o.update({"ps." + k: v for k, v in ps.items()})
    o.update({"res." + k: v for k, v in res.items()})
    o.update({"last." + k: v for k, v in lr.items()})
    o["E"] = np.array([ba.linearizeAll(reset=True)])
    o["opt"] = ba.optimize(3)[1]
    return o


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "st.handles":  # a bijection: positions correspond, no handle twice
            assert len(a[k]) == len(b[k]) == len(set(a[k])) == len(set(b[k])), k
        else:
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def device_path(bs, s, order="scene", compact=True, first=0, drop_first=False, n_imm=None, quality=None,
                cmad=CMAD, capacity=2000):
    ba, frames = build_window(bs, first, drop_first, capacity)
    tr = build_tracer(s, n_imm, quality)
    od = s.order if isinstance(order, str) and n_imm is None else (None if isinstance(order, str) else order)
    r = tr.activate_into(ba, s.slots[frames], s.flagged[frames], cmad, order=od, compact=compact,
                         drop_slot=drop_flags(s, frames))
    r["inputs"] = tr.act_inputs(ba)
    r["dist"] = tr.distance_map()
    return ba, tr, frames, r


def host_path(bs, s, inputs, order="scene", compact=True, first=0, drop_first=False, n_imm=None, quality=None,
              cmad=CMAD):
    """Today's calls."""
    ba, frames = build_window(bs, first, drop_first)
    tr = build_tracer(s, n_imm, quality)
    od = s.order if isinstance(order, str) and n_imm is None else (None if isinstance(order, str) else order)
    i = inputs
    r = tr.activatePointsMT(i["K4"], i["frames"], i["pairs"], i["act_frame"], i["act_u"], i["act_v"], i["act_idepth"],
                            len(i["act_u"]), cmad, od)
    r["dist"] = tr.distance_map()
    a = r["activated"]
    pts = tr.points()
    n = tr.n
    win = {f: k for k, f in enumerate(frames)}
    hd = ba.insertPoints([win[f] for f in s.imm_frame[a]], s.imm_u[a], s.imm_v[a], r["idepth"][a], r["idepth"][a],
                         pts["color"][a].reshape(-1, 8), pts["weights"][a].reshape(-1, 8))
    rh, rt = [], []
    for k, p in enumerate(a):
        for t in range(len(frames)):
            if (r["res_in"][p] >> t) & 1:
                rh.append(hd[k])
                rt.append(t)
    ba.insertResiduals(rh, rt)
    if compact and n:
        keep = (r["action"] == 0) & (drop_flags(s, frames)[s.slots[s.imm_frame[:n]]] == 0)
        tr.compact(keep.astype(np.uint8))
    r["handles"] = hd
    return ba, tr, frames, r


def assert_conditions(s, r, frames):
    """The conditions every test stands on, on the reference (host) path's result."""
    a = r["activated"]
    assert len(a) >= 20 and (r["action"] == 1).sum() >= 20 and (r["action"] == 0).sum() >= 20
    assert len(np.unique(s.imm_frame[a])) >= 3
    assert len({bin(int(x)).count("1") for x in r["res_in"][a]}) >= 2


def both_paths(nF, **kw):
    bs, s = scene(nF)
    bd, td, frames, rd = device_path(bs, s, **kw)
    bh, th, _, rh = host_path(bs, s, rd["inputs"], **kw)
    return bs, s, frames, (bd, td, rd), (bh, th, rh)


def assert_paths_equal(s, frames, dev, host, check_conditions=True):
    (bd, td, rd), (bh, th, rh) = dev, host
    if check_conditions:
        assert_conditions(s, rh, frames)
    assert np.array_equal(rd["action"], rh["action"])
    assert rd["currentMinActDist"] == rh["currentMinActDist"]
    assert np.array_equal(rd["dist"], rh["dist"])
    assert rd["n_activated"] == len(rh["activated"]) == len(rd["handles"])
    assert rd["n_deleted"] == int((rh["action"] == 1).sum())
    a, b = readbacks(bd), readbacks(bh)
    assert_same(a, b)
    # the new handles, in toOptimize order, sit where the host path's do
    pos = {h: p for p, h in enumerate(a["st.handles"])}
    posh = {h: p for p, h in enumerate(b["st.handles"])}
    assert [pos[h] for h in rd["handles"]] == [posh[h] for h in rh["handles"]]
    assert td.n == th.n
    pd_, ph = td.points(), th.points()
    for k in ph:
        assert np.array_equal(pd_[k], ph[k], equal_nan=True), k


def test_formed_inputs_are_the_host_helpers_on_the_windows_state():
    """frames / pairs: bit-equal to hs_host_math.h's make_act_* run on the host over the BA's device state; the active
    points: the window's own (host frame, u, v, idepth)."""
    from hslam_amd import _lib
    from hslam_amd.trace import ACT_FRAME_DT, ACT_PAIR_DT
    for nF in (4, 8):
        bs, s = scene(nF)
        ba, frames = build_window(bs)
        st0, ps0 = ba.structure(), ba.point_state()   # commits the pending edits: the layout the activation reads
        tr = build_tracer(s)
        r = tr.activate_into(ba, s.slots[frames], s.flagged[frames], CMAD, order=s.order, compact=False)
        assert r["n_activated"] >= 20 and r["n_deleted"] >= 20
        i = tr.act_inputs(ba)
        blob = ba.debug_state()
        fr, pr = np.zeros(nF, ACT_FRAME_DT), np.zeros(nF * nF, ACT_PAIR_DT)
        buf = C.create_string_buffer(blob, len(blob))
        _lib.check(_lib.load().hs_debug_act_inputs(buf, nF, None, None, None, None, _lib.ptr(fr), _lib.ptr(pr), None))
        fr["slot"], fr["flagged_for_marg"] = s.slots[frames], s.flagged[frames]
        assert i["frames"].tobytes() == fr.tobytes()
        assert i["pairs"].tobytes() == pr.tobytes()
        assert np.any(pr["aff"][:, 1] != 0)
        assert np.array_equal(i["K4"], s.K4)
        sel = bs.pt_host < nF - 1
        assert np.array_equal(i["act_frame"], st0["pt_host"]) and np.array_equal(i["act_frame"], bs.pt_host[sel])
        assert np.array_equal(i["act_idepth"], ps0["idepth"])
        assert np.array_equal(i["act_u"], bs.pt_u[sel]) and np.array_equal(i["act_v"], bs.pt_v[sel])
        # after the next commit the point arrays have moved: the getter says so
        ba.makeIDX()
        with pytest.raises(_lib.HsError):
            tr.act_inputs(ba)
        assert tr.act_inputs(ba, points=False)["frames"].tobytes() == fr.tobytes()


@pytest.mark.parametrize("nF", [4, 8])
def test_window_and_tracer_equal_the_host_path(nF):
    from test_act import compare, oracle_tracer
    bs, s, frames, dev, host = both_paths(nF)
    assert_paths_equal(s, frames, dev, host)
    # the oracle, through the existing comparison, on the inputs the device formed
    i, rh = dev[2]["inputs"], host[2]
    o = oracle_tracer(s)
    ro = o.activatePointsMT(s.imgs, i["K4"], i["frames"], i["pairs"], i["act_frame"], i["act_u"], i["act_v"],
                            i["act_idepth"], len(i["act_u"]), CMAD, s.order)
    compare(rh, ro, len(s.imm_u))
    assert np.array_equal(dev[2]["dist"], o.distance_map())
    assert np.array_equal(dev[2]["action"], ro["action"])


def test_compact_device_alone_equals_compact():
    bs, s = scene(4)
    rng = np.random.default_rng(5)
    keep = (rng.random(len(s.imm_u)) < 0.6).astype(np.uint8)
    drop = np.zeros(64, np.uint8)
    drop[int(s.slots[1])] = 1
    a, b = build_tracer(s), build_tracer(s)
    assert a.compact_device(keep, drop) == int((keep.astype(bool) & (s.imm_frame != 1)).sum())
    b.compact((keep.astype(bool) & (s.imm_frame != 1)).astype(np.uint8))
    assert a.n == b.n and 20 <= a.n < len(s.imm_u) - 20
    pa, pb = a.points(), b.points()
    for k in pb:
        assert np.array_equal(pa[k], pb[k], equal_nan=True), k
    # a second compaction (the buffer sets have swapped), nothing kept, and no flags without an activation
    keep2 = (rng.random(a.n) < 0.5).astype(np.uint8)
    a.compact_device(keep2)
    b.compact(keep2)
    pa, pb = a.points(), b.points()
    for k in pb:
        assert np.array_equal(pa[k], pb[k], equal_nan=True), k
    from hslam_amd._lib import HsError
    with pytest.raises(HsError):
        a.compact_device(None)
    assert a.compact_device(np.zeros(a.n, np.uint8)) == 0 and a.points()["status"].shape == (0,)


def test_pending_edits():
    """Frames 0-3 committed with their points; then, all uncommitted: frame 0's points removed,
    hs_ba_remove_frame(0, 0), frame 4 inserted, hs_ba_add_residuals_to_newest.  The activation runs over frames 1-4
    with frame 0's slot in drop_slot."""
    bs, s, frames, dev, host = both_paths(5, drop_first=True)
    assert frames == [1, 2, 3, 4]
    assert_paths_equal(s, frames, dev, host)
    # frame 0's immature points were untouched by the activation and left with the compaction
    assert np.all(dev[2]["action"][s.imm_frame == 0] == 0)
    assert dev[1].n == int(((dev[2]["action"] == 0) & (s.imm_frame != 0)).sum())


@pytest.mark.parametrize("case", ["storage_order", "subset_order", "no_compact", "no_immature", "large_cmad",
                                  "none_activated"])
def test_edge_cases(case):
    bs, s = scene(4)
    kw, cond = {}, True
    if case == "storage_order":
        kw = dict(order=None)
    elif case == "subset_order":
        kw = dict(order=s.order[::2].copy())
    elif case == "no_compact":
        kw = dict(compact=False)
    elif case == "no_immature":
        kw, cond = dict(n_imm=0), False
    elif case == "large_cmad":
        # the update rule clamps currentMinActDist to [0, 4], which stops no activation in this scene ...
        kw = dict(cmad=1000.0)
    else:
        # ... so the empty toOptimize list is reached through the trace quality: no point can activate
        kw, cond = dict(quality=np.zeros(len(s.imm_u), np.float32)), False
    _, _, frames, dev, host = both_paths(4, **kw)
    assert_paths_equal(s, frames, dev, host, check_conditions=cond)
    if case == "no_compact":
        assert dev[1].n == len(s.imm_u)
    if case == "no_immature":
        assert dev[2]["n_activated"] == 0 and dev[1].n == 0
    if case == "large_cmad":
        assert dev[2]["currentMinActDist"] == 4.0
    if case == "none_activated":
        assert dev[2]["n_activated"] == 0 and dev[2]["n_deleted"] >= 20 and dev[1].n >= 20


def test_errors_are_loud_and_change_nothing():
    from hslam_amd._lib import HsError
    from hslam_amd.ba import BAWindow
    bs, s = scene(4)
    # capacity overflow: HS_ERR_NOMEM, the window and the tracer as they were
    n_win = int((bs.pt_host < 3).sum())
    ba, frames = build_window(bs, capacity=n_win + 10)
    tr = build_tracer(s)
    st0, p0 = ba.structure(), tr.points()
    with pytest.raises(HsError, match=r"\(-6\)"):
        tr.activate_into(ba, s.slots[frames], s.flagged[frames], CMAD, order=s.order)
    st1, p1 = ba.structure(), tr.points()
    assert tr.n == len(s.imm_u) and all(np.array_equal(st0[k], st1[k]) for k in st0)
    assert all(np.array_equal(p0[k], p1[k], equal_nan=True) for k in p0)
    # a window of another size, a slot without an image, a multi-rank context
    ba, frames = build_window(bs)
    with pytest.raises(HsError, match=r"\(-1\)"):
        tr.activate_into(ba, s.slots[frames[1:]], s.flagged[frames[1:]], CMAD)
    bad = s.slots[frames].copy()
    bad[1] = 60
    with pytest.raises(HsError, match=r"\(-1\)"):
        tr.activate_into(ba, bad, s.flagged[frames], CMAD)
    grp = BAWindow.rank_group([bs.shard(0, 2), bs.shard(1, 2)])
    with pytest.raises(HsError, match=r"\(-5\)"):
        tr.activate_into(grp.members[0], s.slots, s.flagged, CMAD)
    grp.close()
    # the pair still works after the failed calls
    r = tr.activate_into(ba, s.slots[frames], s.flagged[frames], CMAD, order=s.order)
    assert r["n_activated"] >= 20


def test_six_fresh_pairs_give_the_same_bits():
    """No host synchronisation orders the BA's stream and the tracer's: only the events do."""
    bs, s = scene(4)
    ref = None
    for k in range(6):
        ba, tr, frames, r = device_path(bs, s)
        got = readbacks(ba)
        got["action"], got["dist"] = r["action"], r["dist"]
        got.update({"tr." + k2: v for k2, v in tr.points().items()})
        if ref is None:
            ref = got
            assert r["n_activated"] >= 20 and r["n_deleted"] >= 20 and tr.n >= 20
        else:
            assert ref.keys() == got.keys()
            for k2 in ref:
                assert np.array_equal(ref[k2], got[k2], equal_nan=True), (k, k2)
        ba.close()
        tr.close()


def test_lifetime():
    from hslam_amd import _lib
    from hslam_amd._lib import HsError
    lib = _lib.load()
    lib.hs_debug_live_allocations.argtypes, lib.hs_debug_live_allocations.restype = [], C.c_longlong
    bs, s = scene(4)
    gc.collect()  # windows and tracers of earlier tests
    start = lib.hs_debug_live_allocations()
    ba, tr, frames, r = device_path(bs, s)
    assert r["n_activated"] >= 20 and lib.hs_debug_live_allocations() > start
    ba.makeIDX()
    ba.close()
    tr.close()
    assert lib.hs_debug_live_allocations() == start
    # after a failed call
    n_win = int((bs.pt_host < 3).sum())
    ba, frames = build_window(bs, capacity=n_win + 10)
    tr = build_tracer(s)
    with pytest.raises(HsError):
        tr.activate_into(ba, s.slots[frames], s.flagged[frames], CMAD, order=s.order)
    ba.close()
    tr.close()
    assert lib.hs_debug_live_allocations() == start
