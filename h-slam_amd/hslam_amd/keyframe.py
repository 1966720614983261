"""The keyframe path of the BA through the incremental C-ABI: System::AddKeyframe's BA part (Src/Mapping.cpp:12-140).

A synthetic keyframe *sequence* (``make_ba_sequence``: the C4 / C5 scenes' planes, a camera translating along x) and a
driver (``KeyframeBA``) that runs, per keyframe, what AddKeyframe does around the BA:

    insertFrame + setPrecalcValues                     hs_ba_insert_frame (image from the device or a raw upload)
    new residuals of the old points into the new KF    hs_ba_add_residuals_to_newest
    activatePointsMT's new points and residuals        hs_ba_insert_points / hs_ba_insert_residuals
    makeIDX + optimize(6) + the tail                   hs_ba_optimize / hs_ba_fix_linearization
    linearizeAll(true)'s toRemove, removeOutliers      hs_ba_drop_inactive_residuals / _remove_points_without_residuals
    setCoarseTrackingRef (optional tracker)            hs_tracker_set_ref_ba (device hand-off)
    flagPointsForRemoval + marginalizePointsF          (decisions here, System code) + hs_ba_marginalize_points /
                                                       hs_ba_remove_points
    marginalizeFrame                                   hs_ba_remove_frame(marginalize=1)

The System-level decisions (which frame to marginalize, flagPointsForRemoval's per-point tests, the lastResiduals
bookkeeping) are the caller's code in the reference too; they run here in numpy and are not part of the timed library
work.  KeyframeBA(decisions="device") hands flagPointsForRemoval to the library instead: one
hs_ba_flag_points_for_removal call decides on the device (the context keeps lastResiduals itself), runs
marginalizePointsF and removes the points; that call is timed with the library work.  Frame policy: the window holds ``window`` keyframes during optimize and the oldest is marginalized afterwards
(flagFramesForMarginalization's steady state).  KeyframeBA(map=PointMap(...)) attaches a point map (include/hs_map.h): every
point that leaves the window leaves a record there.  KeyframeBA(frame_policy="reference") takes the frames to
marginalize from hs_ba_flag_frames_for_marginalization instead (the reference's point-count, affine and distance-score
rules, with the map's counters; maxFrames = ``window``); it needs a map and decisions="device".

KeyframeBA(points="traced") replaces the invented points by traced ones, the whole chain on the device in the
reference's order (needs decisions="device" and the "oldest" frame policy): the camera frame as one DeviceImage, shared
by every consumer; traceNewCoarse against the window (ImmatureTracer.trace_ba: the hosts' KRKi / Kt / aff formed from the
window's frames on the device); insertFrame with the image handed over on the device; activatePointsMT into the window
(ImmatureTracer.activate_into, the driver keeps currentMinActDist); after flagPointsForRemoval, makeNewTraces on the
new keyframe (PixelSelector.makeMapsImage, FeatureExtractor, ImmatureTracer.add_keys); marginalizeFrame.  trace_frame(k)
is ProcessNonKeyframe: the frame and trace_ba.  A frame's tracer slot is its sequence index modulo 64.  The first
window (bootstrap) still takes candidate points, so that it is well conditioned, and traces keys beside them.
handoff="host" is the same chain with hs_tracer_trace fed ready hs_trace_host arrays (``trace_feed``: what a
handoff="device" run recorded from trace_inputs() with record_inputs=True), the twin of tests and timing.
Two things differ from a literal reading of the reference's steps.  A marginalized frame's immature points leave the
tracer at once (ImmatureTracer.compact_device with the frame's slot in drop_slot), not with the next activation's
compaction: trace_ba refuses points on a slot that is no window frame's, and non-keyframes are traced in between.  The
extractor reads cvImgL as an 8-bit host image (extract_selected on the selector's device map), since a DeviceImage set
from a float frame holds none.
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass

import numpy as np

from .ba import BAWindow, make_frame
from .scene import (PATTERN, SEED, _select_points, make_dir_pyramid, make_plane, pyramid_levels, render,
                    render_depth_at, rodrigues, se3_data, se3_from_data)

RES_IN, RES_OOB, RES_OUT = 0, 1, 2
MIN_GOOD_ACTIVE_RES_FOR_MARG = 3   # setting_minGoodActiveResForMarg (Src/Settings.cpp:96)
MIN_GOOD_RES_FOR_MARG = 4          # setting_minGoodResForMarg (:97)
MIN_IDEPTH_H_MARG = 50.0           # setting_minIdepthH_marg (:119)


@dataclass
class BASequence:
    width: int
    height: int
    K: np.ndarray
    n_levels: int
    poses: np.ndarray        # [N, 7] true worldToCam
    evals: np.ndarray        # [N, 7] the poses the BA starts from (noisy, frame 0 exact)
    raw: list                # [N] (h, w) float32 level-0 images (ImageData::fImgL)
    pyr0: list               # [N] (h, w, 3) float32 DirPyr[0]
    cand: list               # [N] dict(u, v, idepth, idepth_true, color [n, 8], weights [n, 8]): points hosted there
    planes: list = None      # the scene (render_depth_at's truth for points the sequence did not plant)

    @property
    def n_frames(self):
        return len(self.raw)


def make_ba_sequence(n_kf: int = 12, points_per_kf: int = 250, width: int = 640, height: int = 480, K=None,
                     seed: int = SEED, baseline: float = 0.06, max_rot_deg: float = 1.0, pose_noise=(0.004, 0.002),
                     idepth_noise: float = 0.01, kitti: bool = False) -> BASequence:
    """n_kf keyframes of the C4 scene (C5's at KITTI size with kitti=True): camera i at x = baseline * i."""
    rng = np.random.default_rng(seed)
    if K is None:
        K = (np.array([[718.856, 0, 615.5], [0, 718.856, 183.5], [0, 0, 1.0]]) if kitti else
             np.array([[256.0, 0, 319.5], [0, 254.4, 239.5], [0, 0, 1.0]]))
    K = np.asarray(K, np.float64)
    f = K[0, 0]
    if kitti:  # the C4 perturbations in pixels (scene.make_ba_scene_kitti)
        s = 256.0 / f
        pose_noise = (pose_noise[0] * s, pose_noise[1] * s)
        idepth_noise *= s
    planes = [make_plane(rng, 5.0, f), make_plane(rng, 3.0, f, xmax=-0.25 + baseline * n_kf),
              make_plane(rng, 2.0, f, xmin=0.55, ymax=0.15)]
    levels = pyramid_levels(width, height)
    poses, evals, raws, pyrs, cands = [], [], [], [], []
    for i in range(n_kf):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        R_c2w = rodrigues(ax * math.radians(rng.uniform(0, max_rot_deg)))
        C = np.array([baseline * i, 0.0, 0.0])
        img, _ = render(planes, K, R_c2w, C, width, height)
        pyr = make_dir_pyramid(img, 1)
        R_w2c = R_c2w.T
        t_w2c = -R_w2c @ C
        poses.append(se3_data(R_w2c, t_w2c))
        if i == 0:
            evals.append(se3_data(R_w2c, t_w2c))
        else:
            dR = rodrigues(rng.normal(size=3) * pose_noise[1])
            dt = rng.normal(size=3) * pose_noise[0]
            evals.append(se3_data(dR @ R_w2c, dR @ t_w2c + dt))
        raws.append(img)
        pyrs.append(pyr[0])
        pix = _select_points(pyr[0], points_per_kf, 4, rng)
        _, depth = render_depth_at(planes, K, R_c2w, C, pix)
        smp = pyr[0][pix[:, 0:1] + PATTERN[None, :, 1], pix[:, 1:2] + PATTERN[None, :, 0]]
        gx, gy = smp[..., 1], smp[..., 2]
        c2500 = np.float32(2500.0)
        wgt = np.sqrt(c2500 / (c2500 + (gx * gx + gy * gy))).astype(np.float32)
        it = 1.0 / depth
        cands.append(dict(u=pix[:, 1].astype(np.float32), v=pix[:, 0].astype(np.float32),
                          idepth=(it * (1.0 + idepth_noise * rng.normal(size=len(pix)))).astype(np.float32),
                          idepth_true=it, color=np.ascontiguousarray(smp[..., 0], np.float32),
                          weights=np.ascontiguousarray(wgt)))
    return BASequence(width=width, height=height, K=K, n_levels=levels, poses=np.array(poses), evals=np.array(evals),
                      raw=raws, pyr0=pyrs, cand=cands, planes=planes)


def in_bounds_targets(seq: BASequence, host: int, targets, u, v, idepth):
    """[n, len(targets)] bool: the point's centre projects inside the image of each target (evalPT poses), the
    residual set the activation's optimizeImmaturePoint keeps IN on a photo-consistent scene."""
    K = seq.K
    hom = np.stack([u, v, np.ones_like(u)], 1).astype(np.float64) @ np.linalg.inv(K).T
    Rh, th = se3_from_data(seq.evals[host])
    out = np.zeros((len(u), len(targets)), bool)
    for j, t in enumerate(targets):
        if t == host:
            continue
        Rt, tt = se3_from_data(seq.evals[t])
        R = Rt @ Rh.T
        tr = tt - R @ th
        q = hom @ R.T + tr[None, :] * idepth[:, None].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ku = K[0, 0] * q[:, 0] / q[:, 2] + K[0, 2]
            kv = K[1, 1] * q[:, 1] / q[:, 2] + K[1, 2]
        out[:, j] = (q[:, 2] > 0) & (ku > 5.0) & (ku < seq.width - 6) & (kv > 5.0) & (kv < seq.height - 6)
    return out


class _Timer:
    """Wall time spent inside library calls, per phase (the driver's own numpy bookkeeping excluded)."""

    def __init__(self):
        self.t = {}
        self.calls = {}  # per library call (phase/function name)

    def run(self, phase, fn, *a, **k):
        t0 = time.perf_counter()
        r = fn(*a, **k)
        dt = time.perf_counter() - t0
        self.t[phase] = self.t.get(phase, 0.0) + dt
        name = f"{phase}/{getattr(fn, '__name__', 'call')}"
        self.calls[name] = self.calls.get(name, 0.0) + dt
        return r


class KeyframeBA:
    """System::AddKeyframe's BA part over a BASequence, through the incremental C-ABI (module docstring)."""

    def __init__(self, seq: BASequence, device: int = 0, window: int = 8, capacity: int = 0, params=None,
                 tracker=None, image_path: str = "raw", iters: int = 6, allow_break: bool = False,
                 decisions: str = "host", map=None, frame_policy: str = "oldest", points: str = "candidates",
                 handoff: str = "device", key_density: float = 600.0, max_keys: int = 2000, trace_feed=None,
                 record_inputs: bool = False, trace_counts: bool = True):
        if decisions not in ("host", "device"):
            raise ValueError("decisions must be 'host' or 'device'")
        if points not in ("candidates", "traced"):
            raise ValueError("points must be 'candidates' or 'traced'")
        if handoff not in ("device", "host"):
            raise ValueError("handoff must be 'device' or 'host'")
        if points == "traced" and (decisions != "device" or frame_policy != "oldest"):
            raise ValueError("points='traced' needs decisions='device' and frame_policy='oldest'")
        if points == "traced" and handoff == "host" and trace_feed is None:
            raise ValueError("handoff='host' needs trace_feed (a handoff='device' run's recorded trace_inputs)")
        if frame_policy not in ("oldest", "reference"):
            raise ValueError("frame_policy must be 'oldest' or 'reference'")
        if frame_policy == "reference" and (map is None or decisions != "device"):
            raise ValueError("frame_policy='reference' needs a map and decisions='device'")
        # flagPointsForRemoval: "host" decides here in numpy from read-backs (the module docstring's caller code);
        # "device" is one hs_ba_flag_points_for_removal call (the library keeps lastResiduals itself)
        self.decisions = decisions
        self.seq = seq
        self.window = window
        self.iters = iters
        # System::optimize's canbreak (Src/FullSystemOptimize.cpp:493), tested on the device; off by default so that
        # a parity run's iteration count cannot flip on a borderline step norm
        self.allow_break = allow_break
        self.tracker = tracker
        self.image_path = image_path
        ppk = len(seq.cand[0]["u"])
        cap = capacity or ppk * (window + 2) + 64 + (max_keys * window if points == "traced" else 0)
        self.ba = BAWindow(camera=(seq.width, seq.height, seq.n_levels, seq.K), capacity=cap, device=device,
                           params=params)
        # the point map the window's removals append to (None: none, today's path), and who picks the frame to
        # marginalize: "oldest" (frame 0 once the window is full) or "reference" (flagFramesForMarginalization)
        self.map = map
        self.frame_policy = frame_policy
        self.frame_params = None
        if map is not None:
            self.ba.attachMap(map)
        if frame_policy == "reference":  # the reference's settings with the driver's window size
            from .map import frame_marg_params
            self.frame_params = frame_marg_params(maxFrames=window, minFrames=min(5, window - 1))
        self.frames = []                 # window frames as sequence indices (frameHessians order)
        self.cand_of = {}                # handle -> (host sequence index, candidate index)
        self.last_state = {}             # handle -> [lastResiduals[0].second, [1].second] (System bookkeeping)
        self.history = []
        # the traced chain (module docstring): one device frame and its consumers
        self.points = points
        self.handoff = handoff
        self.traced = points == "traced"
        if self.traced:
            from .extract import FeatureExtractor
            from .image import DeviceImage
            from .select import PixelSelector
            from .trace import ImmatureTracer
            self.key_density = key_density
            self.trace_feed = trace_feed          # handoff="host": hs_trace_host arrays, one per trace, in call order
            self.feed_pos = 0
            self.record_inputs = record_inputs    # handoff="device": keep trace_inputs() of every trace in trace_log
            self.trace_log = []
            self.trace_counts = trace_counts
            self.currentMinActDist = 2.0          # System::currentMinActDist's initial value
            self.img = DeviceImage(seq.width, seq.height, seq.n_levels, device)
            self.selector = PixelSelector(seq.width, seq.height, params, device)
            # a descriptor sampling pattern (any will do: the chain reads the keys' positions only)
            pattern = np.random.default_rng(7).integers(-13, 14, size=(256, 2, 2), dtype=np.int8)
            self.extractor = FeatureExtractor(seq.width, seq.height, max_keys, pattern, device)
            self.tracer = ImmatureTracer(seq.width, seq.height, max_keys * (window + 2), device, params)
            self.trace_history = []

    def close(self):
        """Release the window and, in traced mode, the frame and its consumers."""
        if self.traced:
            self.tracer.close()
            self.extractor.close()
            self.selector.__del__()
            self.img.close()
        self.ba.close()

    # ---------------------------------------------------------------- the traced chain
    @staticmethod
    def slot_of(k):
        return int(k) % 64

    def _set_frame(self, k, timer):
        """The camera frame on the device, and the tracer's frame to trace on."""
        timer.run("frame", self.img.set_raw, self.seq.raw[k])
        timer.run("frame", self.tracer.set_frame_image, self.img)

    def _trace(self, k, timer):
        """traceNewCoarse(k) against the window as it stands; returns the status counts (None without trace_counts)."""
        slots = [self.slot_of(f) for f in self.frames]
        if self.handoff == "device":
            c = timer.run("trace", self.tracer.trace_ba, self.ba, slots, self.seq.evals[k], (0.0, 0.0), 1.0,
                          self.trace_counts)
            if self.record_inputs:
                self.trace_log.append(self.tracer.trace_inputs())
        else:
            hosts = self.trace_feed[self.feed_pos]
            self.feed_pos += 1
            c = timer.run("trace", self.tracer.trace_hosts, hosts, self.trace_counts)
        self.trace_history.append(dict(frame=k, n_hosts=len(slots), n_points=self.tracer.n,
                                       counts=None if c is None else c.copy()))
        return c

    def _make_new_traces(self, k, timer, set_image=True):
        """System::makeNewTraces(k): the selector's map and the extractor's keys of the frame in self.img, one
        immature point per key on the frame's slot (set_image: the slot's DirPyr[0] is not there yet)."""
        slot = self.slot_of(k)
        img8 = np.clip(np.rint(self.seq.raw[k]), 0, 255).astype(np.uint8)
        timer.run("new_traces", self.selector.makeMapsImage, self.img, k, self.key_density, 1, 1.0, False)
        timer.run("new_traces", self.extractor.extract_selected, self.selector, img8)
        if set_image:
            timer.run("new_traces", self.tracer.set_host_image_from, slot, self.img)
        return timer.run("new_traces", self.tracer.add_keys, self.extractor, slot)

    def _drop_frame_points(self, k, timer):
        """marginalizeFrame(k)'s immature points: the frame's slot through drop_slot, compacted on the device."""
        drop = np.zeros(64, np.uint8)
        drop[self.slot_of(k)] = 1
        before = self.tracer.n
        timer.run("post", self.tracer.compact_device, np.ones(before, np.uint8), drop)
        return before - self.tracer.n

    def trace_frame(self, k):
        """ProcessNonKeyframe(k): the frame and traceNewCoarse, nothing else.  Returns dict(counts, lib_s)."""
        timer = _Timer()
        self._set_frame(k, timer)
        c = self._trace(k, timer)
        return dict(counts=c, phase_s=dict(timer.t), lib_s=sum(timer.t.values()))

    # ---------------------------------------------------------------- helpers
    def _frame(self, k):
        s = self.seq
        return make_frame(s.evals[k], exposure=1.0, energyTH=8 * 8 * 8, fid=k)

    def _insert_frame(self, k, timer):
        ba = self.ba
        if self.image_path == "host":
            timer.run("setup", ba.insertFrame, self._frame(k), image=self.seq.pyr0[k])
        elif self.image_path in ("device", "device_ptr") and self.tracker is not None:
            # the frame was tracked before it became a keyframe: its pyramid is already on the device (tracking
            # work, reported apart from the BA's)
            timer.run("track_frame", self.tracker.set_frame_raw, self.seq.raw[k])
            if self.image_path == "device_ptr":  # through the texels' address (hs_ba_set_frame_image_device)
                timer.run("setup", ba.insertFrame, self._frame(k), device_texels=self.tracker.frame_texels(0))
            else:
                timer.run("setup", ba.insertFrame, self._frame(k), tracker=self.tracker)
        else:
            timer.run("setup", ba.insertFrame, self._frame(k), raw=self.seq.raw[k])
        self.frames.append(k)

    def _activate(self, host_k, timer, cand_idx=None):
        """activatePointsMT's result for the points hosted by sequence frame host_k: insertPoint + insertResidual
        into every other window frame the centre projects into."""
        c = self.seq.cand[host_k]
        idx = np.arange(len(c["u"])) if cand_idx is None else np.asarray(cand_idx)
        h = self.frames.index(host_k)
        ok = in_bounds_targets(self.seq, host_k, self.frames, c["u"][idx], c["v"][idx], c["idepth"][idx])
        keep = ok.sum(1) > 0
        idx, ok = idx[keep], ok[keep]
        handles = timer.run("setup", self.ba.insertPoints, np.full(len(idx), h, np.int32), c["u"][idx], c["v"][idx],
                            c["idepth"][idx], c["idepth"][idx], c["color"][idx], c["weights"][idx])
        pi, ti = np.nonzero(ok)
        timer.run("setup", self.ba.insertResiduals, handles[pi], ti.astype(np.int32))
        newest, second = len(self.frames) - 1, len(self.frames) - 2
        for j, hd in enumerate(handles):
            self.cand_of[int(hd)] = (host_k, int(idx[j]))
            if self.decisions == "host":
                self.last_state[int(hd)] = [RES_IN if ok[j, newest] else RES_OOB,
                                            RES_IN if second >= 0 and ok[j, second] else RES_OOB]
        return handles

    # ---------------------------------------------------------------- the sequence
    def bootstrap(self, n_frames=None):
        """The first window: keyframes 0 .. n-1 with the points of frames 0 .. n-2 (the newest KF's points activate
        with the next keyframe, as in the steady state).  In traced mode the window is built the same way, from
        candidate points, and every bootstrap frame also gets its keys as immature points, traced on the later
        bootstrap frames."""
        n = n_frames or self.window - 1
        timer = _Timer()
        for k in range(n):
            self._insert_frame(k, timer)
        for k in range(n - 1):
            self._activate(k, timer)
        self.ba.makeIDX()
        if self.traced:
            # every bootstrap keyframe traced on the later ones as they come, then makeNewTraces on it: at frame k the
            # tracer holds the points of frames < k (the window's later frames get records no point reads)
            for k in range(n):
                self._set_frame(k, timer)
                if k > 0:
                    self._trace(k, timer)
                self._make_new_traces(k, timer)

    def add_keyframe(self, k, marginalize=True, check=None):
        """AddKeyframe(k)'s BA part.  check(driver, phase) is called at 'optimize' (before it), 'tail' (after the
        tail, before its drops), and with marginalization at 'marginalize' (before marginalizePointsF of
        self.marg_points), 'points_marginalized' (after it) and 'frame_marginalized' (after marginalizeFrame of
        self.marg_frame): parity tests rebuild the window there.  Returns dict of per-phase seconds."""
        ba, timer = self.ba, _Timer()
        host_rule = self.decisions == "host"
        wall0 = time.perf_counter()
        traced_info = {}
        if self.traced:
            # the camera frame, traceNewCoarse, insertFrame with the frame's image handed over on the device, the old
            # points' residuals, activatePointsMT of the traced points into the window
            self._set_frame(k, timer)
            counts = self._trace(k, timer)
            idx = timer.run("setup", ba.insertFrame, self._frame(k))
            timer.run("setup", ba.set_frame_image_from, idx, self.img)
            # the keyframe's DirPyr[0] in its tracer slot: the activation's residuals into it read it there
            timer.run("setup", self.tracer.set_host_image_from, self.slot_of(k), self.img)
            self.frames.append(k)
            timer.run("setup", ba.addResidualsToNewest)
            flagged = np.zeros(len(self.frames), np.int32)
            if marginalize and len(self.frames) >= self.window:
                flagged[0] = 1   # the frame this keyframe will marginalize
            n_imm = self.tracer.n
            act = self.last_activation = timer.run(
                "activate", self.tracer.activate_into, ba, [self.slot_of(f) for f in self.frames], flagged,
                self.currentMinActDist, None, True, None)
            self.currentMinActDist = act["currentMinActDist"]
            traced_info = dict(trace_counts=counts, n_immature=n_imm, n_activated=act["n_activated"],
                               n_deleted=act["n_deleted"], act_handles=act["handles"],
                               currentMinActDist=self.currentMinActDist, imm_dropped_with_frame=0)
        else:
            # insertFrame, new residuals of the old points, activation of the previous newest KF's points
            self._insert_frame(k, timer)
            timer.run("setup", ba.addResidualsToNewest)
            for hd, st in self.last_state.items():
                st[1], st[0] = st[0], RES_IN
            self._activate(self.frames[-2], timer)
        timer.run("setup", ba.makeIDX)
        timer.run("setup", ba.synchronize)
        if check:
            check(self, "optimize")
        # optimize + tail
        n_it, energies = timer.run("optimize", ba.optimize, self.iters, self.allow_break)
        # the per-point maxRelBaseline / numGoodResiduals stay on the device (read with point_state when needed)
        tail = self.last_tail = timer.run("tail", ba.fixLinearization, None, None, False)
        if check:
            check(self, "tail")
        # lastResiduals[.].second from the tail's states (System::linearizeAll(true), Src/FullSystemOptimize.cpp:128)
        if host_rule:
            st = ba.structure()
            res = ba.residuals()
            handles = st["handles"]
            newest, second = len(self.frames) - 1, len(self.frames) - 2
            for r in np.nonzero((st["res_target"] == newest) | (st["res_target"] == second))[0]:
                hd = int(handles[st["res_point"][r]])
                self.last_state[hd][0 if st["res_target"][r] == newest else 1] = int(res["state"][r])
            hdif = tail["HdiF"]
        # toRemove, removeOutliers, the tracker's new reference
        timer.run("post", ba.dropInactiveResiduals)
        gone = timer.run("post", ba.removeOutliers)
        for hd in gone:
            self.cand_of.pop(int(hd), None)
            self.last_state.pop(int(hd), None)
        if self.tracker is not None:
            timer.run("post", self.tracker.set_ref_ba, ba, self.image_path in ("device", "device_ptr"))
        # flagPointsForRemoval (Src/Mapping.cpp:248-328), the frame to marginalize: the oldest once the window is full
        info = dict(energies=energies, iters=n_it, n_points=ba.n_points, n_res=ba.n_res, dropped_points=len(gone))
        info.update(traced_info)
        new_traces_done = False
        if marginalize and self.frame_policy == "reference":
            # flagFramesForMarginalization decides (KfId = the sequence index; the newest keyframe's candidates are its
            # immature points), then flagPointsForRemoval and marginalizeFrame of every flagged frame
            kf_id = np.asarray(self.frames, np.int32)
            n_imm = np.zeros(len(self.frames), np.int32)
            n_imm[-1] = len(self.seq.cand[self.frames[-1]]["u"])
            self.frame_inputs = dict(kf_id=kf_id, n_immature=n_imm)
            if check:
                check(self, "flag_frames")
            fl = self.frame_flags = timer.run("post", ba.flagFramesForMarginalization, kf_id, n_imm, self.frame_params)
            marg_fs = [int(f) for f in np.nonzero(fl)[0]]
            hd_all = ba.structure()["handles"]
            self.marg_points, self.marg_frame, self.marg_frames = None, (marg_fs[0] if marg_fs else None), marg_fs
            if check:
                check(self, "marginalize")
            flg = self.last_flags = timer.run("post", ba.flagPointsForRemoval, marg_fs, True, False)
            marg, drop = flg["action"] == 2, flg["action"] == 1
            self.marg_points = np.nonzero(marg)[0].astype(np.int32)
            self.marg_handles, self.drop_handles = hd_all[marg], hd_all[drop]
            if check:
                check(self, "points_marginalized")
            for hd in hd_all[marg | drop]:
                self.cand_of.pop(int(hd), None)
            for f in reversed(marg_fs):
                timer.run("post", ba.removeFrame, f, True)
                self.frames.pop(f)
            if check:
                check(self, "frame_marginalized")
            info.update(marginalized_points=int(marg.sum()), dropped=int(drop.sum()), marg_frames=marg_fs)
        elif marginalize and len(self.frames) >= self.window and not host_rule:
            # the decisions, marginalizePointsF and the removals in one library call; only the actions come back
            marg_f = 0
            hd_all = ba.structure()["handles"]
            self.marg_points, self.marg_frame = None, marg_f  # the points are known after the call
            if check:
                check(self, "marginalize")
            flg = self.last_flags = timer.run("post", ba.flagPointsForRemoval, [marg_f], True, False)
            marg, drop = flg["action"] == 2, flg["action"] == 1
            self.marg_points = np.nonzero(marg)[0].astype(np.int32)
            self.marg_handles, self.drop_handles = hd_all[marg], hd_all[drop]
            if check:
                check(self, "points_marginalized")
            for hd in hd_all[marg | drop]:
                self.cand_of.pop(int(hd), None)
            if self.traced:  # makeNewTraces(fh) stands between flagPointsForRemoval and marginalizeFrame
                info["n_keys"] = self._make_new_traces(k, timer, set_image=False)
                new_traces_done = True
            timer.run("post", ba.removeFrame, marg_f, True)
            gone_k = self.frames.pop(marg_f)
            if self.traced:
                info["imm_dropped_with_frame"] = self._drop_frame_points(gone_k, timer)
            if check:
                check(self, "frame_marginalized")
            info.update(marginalized_points=int(marg.sum()), dropped=int(drop.sum()))
        elif marginalize and len(self.frames) >= self.window:
            marg_f = 0
            st = ba.structure()
            ps = ba.point_state()
            res = ba.residuals()
            hd_all, host, nres = st["handles"], st["pt_host"], st["nres"]
            # the tail's per-point values in the tail's layout -> by handle (removeOutliers only removed points)
            vis_marg = np.zeros(len(hd_all), np.int32)
            sel = (st["res_target"] == marg_f) & (res["state"] == RES_IN)
            np.add.at(vis_marg, st["res_point"][sel], 1)
            last0 = np.array([self.last_state[int(h)][0] for h in hd_all])
            last1 = np.array([self.last_state[int(h)][1] for h in hd_all])
            ng = ps["numGoodResiduals"]
            oob = ((nres >= MIN_GOOD_ACTIVE_RES_FOR_MARG) & (ng > MIN_GOOD_RES_FOR_MARG + 10) &
                   (nres - vis_marg < MIN_GOOD_ACTIVE_RES_FOR_MARG))
            oob |= last0 == RES_OOB
            oob |= (nres >= 2) & (last0 == RES_OUT) & (last1 == RES_OUT)
            flag = oob | (host == marg_f)
            drop_now = (ps["idepth"] < 0) | (nres == 0)
            inl = (nres >= MIN_GOOD_ACTIVE_RES_FOR_MARG) & (ng >= MIN_GOOD_RES_FOR_MARG)
            hdif_now = self._hdif_by_handle(hd_all, tail_handles=handles, hdif=hdif)
            with np.errstate(divide="ignore"):
                idepth_h = np.where(hdif_now > 0, 1.0 / hdif_now, 0.0)
            marg = flag & ~drop_now & inl & (idepth_h > MIN_IDEPTH_H_MARG)
            drop = drop_now | (flag & ~marg)
            mpos = np.nonzero(marg)[0].astype(np.int32)
            self.marg_points, self.marg_frame = mpos, marg_f
            self.marg_handles, self.drop_handles = hd_all[marg], hd_all[drop]
            if check:
                check(self, "marginalize")  # before marginalizePointsF: the window as the tail and drops left it
            if len(mpos):
                timer.run("post", ba.marginalizePointsF, mpos, False)
            if check:
                check(self, "points_marginalized")
            rm = hd_all[marg | drop]
            timer.run("post", ba.removePoints, rm)
            for hd in rm:
                self.cand_of.pop(int(hd), None)
                self.last_state.pop(int(hd), None)
            timer.run("post", ba.removeFrame, marg_f, True)
            self.frames.pop(marg_f)
            if check:
                check(self, "frame_marginalized")
            info.update(marginalized_points=int(marg.sum()), dropped=int(drop.sum()))
        if self.traced and not new_traces_done:
            info["n_keys"] = self._make_new_traces(k, timer, set_image=False)
        timer.run("post", ba.synchronize)
        info["wall_s"] = time.perf_counter() - wall0
        info["phase_s"] = dict(timer.t)
        info["call_s"] = dict(timer.calls)
        info["lib_s"] = sum(v for p, v in timer.t.items() if p != "track_frame")
        self.history.append(info)
        return info

    @staticmethod
    def _hdif_by_handle(hd_now, tail_handles, hdif):
        pos = {int(h): i for i, h in enumerate(tail_handles)}
        return np.array([hdif[pos[int(h)]] for h in hd_now], np.float64)
