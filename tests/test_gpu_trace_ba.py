"""hs_tracer_trace_ba: System::traceNewCoarse whose window is the BA context's -- each host's (KRKi, Kt, aff) formed on
the device from the window's frames -- against hs_tracer_trace fed the arrays hs_tracer_get_trace_inputs returns, and
the keyframe driver's traced chain (KeyframeBA(points="traced")) against its host-fed twin.  Every comparison of the
two hand-offs is bit for bit.

Scene: make_ba_sequence at 320 x 240 (3 pyramid levels), the candidates of each frame as its immature points in the
hand-off tests; the chain takes its points from the selector and the extractor."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 320, 240
K = np.array([[128.0, 0, 159.5], [0, 127.2, 119.5], [0, 0, 1.0]])
NEW_AFF, NEW_EXPO = (0.03, -2.0), 1.3


def slot(k):
    """The hand-off tests' slots: neither contiguous nor in window order."""
    return (5 * k + 3) % 64


@functools.lru_cache(maxsize=None)
def sequence():
    from hslam_amd.keyframe import make_ba_sequence
    return make_ba_sequence(n_kf=6, points_per_kf=120, width=W, height=H, K=K, seed=11)


def frame_of(seq, k, aff):
    """aff: the frame carries a non-zero affine state (a = 10 state[6], b = 1000 state[7]) and its own exposure."""
    from hslam_amd.ba import make_frame
    st = np.zeros(10)
    if aff:
        st[6], st[7] = 0.002 * (k + 1) * (-1) ** k, 0.001 * (k - 1.5)
    return make_frame(seq.evals[k], state=st, exposure=0.8 + 0.15 * k if aff else 1.0, fid=k)


def build_window(seq, frames, committed=None, aff=False):
    """The first `committed` (None: all) of `frames` (sequence indices) inserted and committed, with the candidates
    of every one of them but the last as their points and residuals into the frames they project into; the other
    frames inserted after that commit and left pending.  Returns (window, {frame: its points' handles})."""
    from hslam_amd.ba import BAWindow
    from hslam_amd.keyframe import in_bounds_targets
    ba = BAWindow(camera=(W, H, seq.n_levels, seq.K), capacity=2000)
    win = frames[:len(frames) if committed is None else committed]
    for k in win:
        ba.insertFrame(frame_of(seq, k, aff), image=seq.pyr0[k])
    handles = {}
    for k in win[:-1]:
        c = seq.cand[k]
        ok = in_bounds_targets(seq, k, win, c["u"], c["v"], c["idepth"])
        idx = np.nonzero(ok.sum(1) > 0)[0]
        hd = ba.insertPoints(np.full(len(idx), win.index(k), np.int32), c["u"][idx], c["v"][idx], c["idepth"][idx],
                             c["idepth"][idx], c["color"][idx], c["weights"][idx])
        pi, ti = np.nonzero(ok[idx])
        ba.insertResiduals(hd[pi], ti.astype(np.int32))
        handles[k] = hd
    ba.makeIDX()
    for k in frames[len(win):]:
        ba.insertFrame(frame_of(seq, k, aff), image=seq.pyr0[k])
        ba.addResidualsToNewest()
    return ba, handles


def build_tracer(seq, frames, new):
    from hslam_amd.trace import ImmatureTracer
    tr = ImmatureTracer(W, H, 2000)
    for k in frames:
        tr.set_host_image(slot(k), seq.pyr0[k])
        c = seq.cand[k]
        tr.add_points(np.full(len(c["u"]), slot(k), np.int32), c["u"], c["v"])
    if new is not None:
        tr.set_frame(seq.pyr0[new])
    return tr


def commit_count(ba):
    from hslam_amd import _lib
    return _lib.load().hs_debug_commit_count(ba.h)


def host_inline(blob, nF, idx, pose7, aff, expo):
    """hs_debug_trace_hosts on a window's read-back device state (BAWindow.debug_state(), which commits what is
    pending) -> [nF, 14] float32 in frame order."""
    from hslam_amd import _lib
    buf = C.create_string_buffer(blob, len(blob))
    out = np.zeros((nF, 14), np.float32)
    ix = None if idx is None else np.ascontiguousarray(idx, np.int32)
    p, a = np.ascontiguousarray(pose7, np.float64), np.ascontiguousarray(aff, np.float64)
    _lib.check(_lib.load().hs_debug_trace_hosts(buf, nF, _lib.ptr(ix), None, None, None, None, _lib.ptr(p), _lib.ptr(a),
                                                float(expo), _lib.ptr(out)))
    return out


def same_points(a, b, fields=None):
    for k in (fields or a.keys()):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_formed_inputs_are_the_host_inline_on_the_windows_state():
    seq = sequence()
    frames, new = [0, 1, 2, 3], 4
    slots = [slot(k) for k in frames]
    # zero affine states, unit exposures: exp(0) is exact, every record bit for bit
    ba, _ = build_window(seq, frames)
    tr = build_tracer(seq, frames, new)
    tr.trace_ba(ba, slots, seq.evals[new])
    inp = tr.trace_inputs()
    ref = host_inline(ba.debug_state(), 4, None, seq.evals[new], (0.0, 0.0), 1.0)
    assert inp.shape == (max(slots) + 1, 14)
    assert inp[slots].tobytes() == ref.tobytes()
    assert np.all(inp[slots, 12] == 1.0) and np.all(inp[slots, 13] == 0.0)
    assert not np.any(np.delete(inp, slots, 0))          # nothing formed on the slots of no frame
    assert np.any(inp[slots[:3], 9:12] != 0)
    # non-zero affine states and exposures on poses two GN steps have moved on the device: KRKi / Kt bit for bit,
    # aff within one float ulp (the device's and the host's fp64 exp are each within one fp64 ulp of the exact value,
    # and the cast to float can round the two to neighbouring floats)
    ba2, _ = build_window(seq, frames, aff=True)
    ba2.optimize(2)
    tr2 = build_tracer(seq, frames, new)
    tr2.trace_ba(ba2, slots, seq.evals[new], NEW_AFF, NEW_EXPO)
    inp2 = tr2.trace_inputs()
    ref2 = host_inline(ba2.debug_state(), 4, None, seq.evals[new], NEW_AFF, NEW_EXPO)
    assert inp2[slots][:, :12].tobytes() == ref2[:, :12].tobytes()
    assert np.all(ulps(inp2[slots][:, 12:], ref2[:, 12:]) <= 1)
    assert np.all(ref2[:, 12] != 1.0) and np.all(ref2[:, 13] != 0.0)
    assert inp2[slots][:, :12].tobytes() != inp[slots][:, :12].tobytes()      # the poses did move


def test_trace_equals_hs_tracer_trace_on_the_formed_inputs():
    seq = sequence()
    frames = [0, 1, 2, 3]
    slots = [slot(k) for k in frames]
    assert len(slots) >= 3
    ba, _ = build_window(seq, frames, aff=True)
    ba.optimize(2)
    td, th = build_tracer(seq, frames, None), build_tracer(seq, frames, None)
    seen = set()
    for new in (4, 5):     # the second trace starts from the first one's intervals
        td.set_frame(seq.pyr0[new])
        th.set_frame(seq.pyr0[new])
        cd = td.trace_ba(ba, slots, seq.evals[new], NEW_AFF, NEW_EXPO)
        ch = th.traceNewCoarse(*np.split(td.trace_inputs(), [9, 12], 1))
        assert np.array_equal(cd, ch) and cd.sum() == td.n == th.n
        pd_, ph = td.points(), th.points()
        same_points(pd_, ph)
        assert cd[0] >= 20                                    # IPS_GOOD
        seen |= set(np.nonzero(cd)[0].tolist())
    assert len(seen) >= 2
    # without the counts the call does not wait; the points are the same
    t3 = build_tracer(seq, frames, 4)
    assert t3.trace_ba(ba, slots, seq.evals[4], NEW_AFF, NEW_EXPO, counts=False) is None
    t4 = build_tracer(seq, frames, 4)
    t4.trace_ba(ba, slots, seq.evals[4], NEW_AFF, NEW_EXPO)
    same_points(t3.points(), t4.points())


def test_pending_removals_commit_nothing():
    """Frames 0-3 committed; frame 0's points removed and hs_ba_remove_frame(0) pending: the call reads frames 1-3 at
    their committed indices 1-3 and commits nothing; the traces are those of a window built of frames 1-3 alone."""
    seq = sequence()
    frames, new = [0, 1, 2, 3], 4
    ba, hd = build_window(seq, frames)
    blob = ba.debug_state()
    ba.removePoints(hd[0])
    ba.removeFrame(0, marginalize=False)
    rest = frames[1:]
    slots = [slot(k) for k in rest]
    assert slot(0) not in slots
    tr = build_tracer(seq, rest, new)
    c0 = commit_count(ba)
    cnt = tr.trace_ba(ba, slots, seq.evals[new])
    assert commit_count(ba) == c0
    inp = tr.trace_inputs()
    assert inp[slots].tobytes() == host_inline(blob, 3, [1, 2, 3], seq.evals[new], (0.0, 0.0), 1.0).tobytes()
    ba2, _ = build_window(seq, rest)
    tr2 = build_tracer(seq, rest, new)
    cnt2 = tr2.trace_ba(ba2, slots, seq.evals[new])
    assert np.array_equal(cnt, cnt2) and cnt[0] >= 20
    assert tr2.trace_inputs().tobytes() == inp.tobytes()
    same_points(tr.points(), tr2.points())
    # the pending edits are still the caller's to commit
    ba.makeIDX()
    assert commit_count(ba) == c0 + 1 and ba.nF == 3


def test_a_pending_inserted_frame_is_committed_first():
    seq = sequence()
    frames, new = [0, 1, 2, 3], 4
    slots = [slot(k) for k in frames]
    ba, _ = build_window(seq, frames, committed=3)
    tr = build_tracer(seq, frames, new)
    c0 = commit_count(ba)
    cnt = tr.trace_ba(ba, slots, seq.evals[new])
    assert commit_count(ba) == c0 + 1
    ba2, _ = build_window(seq, frames, committed=3)
    ba2.makeIDX()
    tr2 = build_tracer(seq, frames, new)
    c2 = commit_count(ba2)
    cnt2 = tr2.trace_ba(ba2, slots, seq.evals[new])
    assert commit_count(ba2) == c2
    assert np.array_equal(cnt, cnt2) and cnt[0] >= 20
    assert tr.trace_inputs().tobytes() == tr2.trace_inputs().tobytes()
    same_points(tr.points(), tr2.points())
    assert np.any(tr.points()["status"][-len(seq.cand[3]["u"]):] == 0)     # the inserted frame's points traced too


def test_errors_are_loud_and_change_nothing():
    import torch
    from hslam_amd._lib import HsError
    from hslam_amd.ba import BAWindow
    from hslam_amd.scene import make_ba_scene
    from hslam_amd.trace import ImmatureTracer
    seq = sequence()
    frames, new = [0, 1, 2, 3], 4
    slots = [slot(k) for k in frames]
    ba, _ = build_window(seq, frames, committed=3)      # an inserted frame pending: a commit would show
    tr = build_tracer(seq, frames, new)
    c0, p0 = commit_count(ba), tr.points()

    def unchanged():
        assert commit_count(ba) == c0
        same_points(p0, tr.points())

    # a multi-rank context: HS_ERR_STATE
    bs = make_ba_scene(n_points=160, n_frames=4, width=W, height=H, seed=5)
    grp = BAWindow.rank_group([bs.shard(0, 2), bs.shard(1, 2)])
    with pytest.raises(HsError, match=r"\(-5\)"):
        tr.trace_ba(grp.members[0], slots, seq.evals[new])
    grp.close()
    unchanged()
    # another image size, nF not the window's, a point on a slot that slots does not name: HS_ERR_INVALID
    big = ImmatureTracer(W + 16, H, 16)
    big.set_frame(np.zeros((H, W + 16, 3), np.float32))
    with pytest.raises(HsError, match=r"\(-1\)"):
        big.trace_ba(ba, slots, seq.evals[new])
    big.close()
    with pytest.raises(HsError, match=r"\(-1\)"):
        tr.trace_ba(ba, slots[:3], seq.evals[new])
    unchanged()
    other = slots[:3] + [slot(9)]
    with pytest.raises(HsError, match=r"\(-1\)"):
        tr.trace_ba(ba, other, seq.evals[new])
    with pytest.raises(HsError, match=r"\(-1\)"):
        tr.trace_ba(ba, slots[:3] + [slots[0]], seq.evals[new])
    unchanged()
    # another device (where the machine has one)
    if torch.cuda.device_count() > 1:
        far = ImmatureTracer(W, H, 16, device=1)
        far.set_frame(seq.pyr0[new])
        with pytest.raises(HsError, match=r"\(-1\)"):
            far.trace_ba(ba, slots, seq.evals[new])
        far.close()
        unchanged()
    # no frame set: HS_ERR_STATE
    bare = build_tracer(seq, frames, None)
    pb = bare.points()
    with pytest.raises(HsError, match=r"\(-5\)"):
        bare.trace_ba(ba, slots, seq.evals[new])
    same_points(pb, bare.points())
    unchanged()
    # the pair still works after the failed calls
    assert tr.trace_ba(ba, slots, seq.evals[new])[0] >= 20
    assert commit_count(ba) == c0 + 1


# ---- the keyframe driver's traced chain ---------------------------------------------------------------------------

N_BOOT, N_RUN, WINDOW = 3, 8, 4
CHAIN = dict(window=WINDOW, decisions="device", points="traced", key_density=400.0)


@functools.lru_cache(maxsize=None)
def chain_sequence():
    from hslam_amd.keyframe import make_ba_sequence
    return make_ba_sequence(n_kf=N_BOOT + N_RUN, points_per_kf=150, width=W, height=H, K=K, seed=3, baseline=0.05)


def is_keyframe(k):
    return (k - N_BOOT) % 2 == 1     # every second frame after the first window


def tracer_points(drv):
    return {"tr." + k: v for k, v in drv.tracer.points().items()}


def window_state(ba):
    """The window's read-backs that leave it as it is."""
    st, ps, res, lr = ba.structure(), ba.point_state(), ba.residuals(), ba.lastResiduals()
    o = {"st." + k: v for k, v in st.items()}
    o.update({"ps." + k: v for k, v in ps.items()})
    o.update({"res." + k: v for k, v in res.items()})
    o.update({"last." + k: v for k, v in lr.items()})
    return o


def run_chain(handoff, feed=None, stop_at=None, **kw):
    """The traced chain over chain_sequence(): the first window, then 8 frames, every second one a keyframe.  After
    every keyframe the window's state and the tracer's points are kept; stop_at (a keyframe's sequence index) ends the
    run there with test_gpu_act_ba.py's readbacks (one linearizeAll and optimize(3): they change the window, so each
    keyframe gets a run of its own).  Returns (driver, per-keyframe list, the readbacks or None)."""
    from hslam_amd.keyframe import KeyframeBA
    from test_gpu_act_ba import readbacks
    seq = chain_sequence()
    args = dict(CHAIN, **kw)
    drv = KeyframeBA(seq, handoff=handoff, trace_feed=feed, record_inputs=handoff == "device", **args)
    drv.bootstrap(N_BOOT)
    per_kf = []
    for k in range(N_BOOT, N_BOOT + N_RUN):
        if not is_keyframe(k):
            drv.trace_frame(k)
            continue
        info = drv.add_keyframe(k)
        o = window_state(drv.ba)
        o.update(tracer_points(drv))
        per_kf.append((k, info, o))
        if k == stop_at:
            return drv, per_kf, readbacks(drv.ba)
    return drv, per_kf, None


@functools.lru_cache(maxsize=None)
def full_runs():
    dev, kd, _ = run_chain("device")
    host, kh, _ = run_chain("host", feed=dev.trace_log)
    return dev, kd, host, kh


def test_chain_equals_its_host_fed_twin():
    from test_gpu_act_ba import assert_same
    dev, kd, host, kh = full_runs()
    assert len(kd) == len(kh) == N_RUN // 2
    # the conditions this test stands on, on the host-fed chain alone
    assert sum(i["n_activated"] >= 20 for _, i, _ in kh) >= 3
    assert any(i["n_deleted"] > 0 for _, i, _ in kh)
    assert any(i["imm_dropped_with_frame"] > 0 for _, i, _ in kh)
    assert any(t["counts"][0] > 0 and np.count_nonzero(t["counts"][1:]) > 0 for t in host.trace_history)
    assert any(t["n_hosts"] >= 3 and t["n_points"] > 0 for t in host.trace_history)
    assert host.feed_pos == len(dev.trace_log) == len(host.trace_history)
    for (k, idv, a), (k2, ih, b) in zip(kd, kh):
        assert k == k2
        assert_same(a, b)
        assert idv["n_activated"] == ih["n_activated"] and idv["n_deleted"] == ih["n_deleted"]
        assert idv["currentMinActDist"] == ih["currentMinActDist"] and idv["n_keys"] == ih["n_keys"]
        assert np.array_equal(idv["energies"], ih["energies"])
    for td, th in zip(dev.trace_history, host.trace_history):
        assert np.array_equal(td["counts"], th["counts"]) and td["n_points"] == th["n_points"]
    # one linearizeAll and optimize(3) after every keyframe, each on a run of its own
    for k, _, a in kd:
        d2, kd2, rd = run_chain("device", stop_at=k)
        h2, kh2, rh = run_chain("host", feed=dev.trace_log, stop_at=k)
        assert_same(kd2[-1][2], a)            # the run is the run
        assert_same(rd, rh)
        d2.close()
        h2.close()


def test_chain_is_sane_and_the_candidates_path_is_untouched():
    from hslam_amd.keyframe import KeyframeBA
    from test_gpu_act_ba import assert_same, readbacks
    dev, kd, _, _ = full_runs()
    for k, info, _ in kd:
        e = info["energies"]
        assert np.all(np.isfinite(e)) and e[-1] <= e[0], (k, e)
        assert 200 <= info["n_keys"] <= 450, info["n_keys"]
        assert info["n_points"] > 0 and info["n_res"] > 0
    # the candidates path beside the traced objects, and again from a driver built when none of them is left
    seq = chain_sequence()

    def candidates():
        d = KeyframeBA(seq, window=WINDOW, decisions="device")
        assert not d.traced and not hasattr(d, "tracer")
        d.bootstrap(N_BOOT)
        out = []
        for k in range(N_BOOT, N_BOOT + 3):
            info = d.add_keyframe(k)
            o = window_state(d.ba)
            o["energies"] = info["energies"]
            out.append(o)
        out.append(readbacks(d.ba))
        d.close()
        return out

    beside = candidates()
    dev, _, host, _ = full_runs()
    full_runs.cache_clear()
    dev.close()
    host.close()
    del dev, host, kd
    gc.collect()
    alone = candidates()
    for a, b in zip(beside, alone):
        assert_same(a, b)


def test_lifetime():
    from hslam_amd import _lib
    lib = _lib.load()
    lib.hs_debug_live_allocations.argtypes, lib.hs_debug_live_allocations.restype = [], C.c_longlong
    full_runs.cache_clear()
    gc.collect()  # drivers, windows and tracers of earlier tests
    start = lib.hs_debug_live_allocations()
    drv, per_kf, _ = run_chain("device", stop_at=N_BOOT + 3)
    assert len(per_kf) == 2 and lib.hs_debug_live_allocations() > start
    drv.close()
    del drv, per_kf
    gc.collect()
    assert lib.hs_debug_live_allocations() == start
