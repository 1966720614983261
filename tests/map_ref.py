"""numpy restatements of the two reference functions the point map replaces (include/hs_map.h), shared by
tests/test_frame_rule.py and tests/test_gpu_map.py:

    refresh_pc    KFDisplay::RefreshPC (Src/Display.cpp:382-513) without the z jitter: np.float32 operations in the
                  reference's order, the double literal 0.01 in the variance.
    frame_rule    System::flagFramesForMarginalization (Src/FullSystemMarginalize.cpp:18-103) with the reference's types.
"""
import numpy as np

PATTERN = np.array([[0, -2], [-1, -1], [1, -1], [-2, 0], [0, 0], [2, 0], [-1, 1], [0, 2]], dtype=np.int32)
F32 = np.float32
WHY_POINTS, WHY_AFFINE, WHY_SCORE, WHY_AGE, WHY_BLOCKED = 1, 2, 4, 8, 16


def cloud_keep(idepth, hdif, max_rel_baseline):
    """RefreshPC's per-point filter: (keep mask, depth), and the three filter terms for coverage checks."""
    idepth = np.asarray(idepth, F32)
    hdif = np.asarray(hdif, F32)
    rel = np.asarray(max_rel_baseline, F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        depth = F32(1.0) / idepth
        depth4 = depth * depth
        depth4 = depth4 * depth4
        ih = np.where(hdif > 0, (1.0 / hdif.astype(np.float64)).astype(F32), F32(0))  # idepth_hessian (hs_flag_rule.h)
        var = (1.0 / (ih.astype(np.float64) + 0.01)).astype(F32)
        neg = idepth < 0
        scaled = var * depth4 > F32(0.001)
        absv = var > F32(0.001)
        base = rel < F32(0.1)
    keep = ~neg & ~scaled & ~absv & ~base
    return keep, depth, dict(neg=neg, scaled=scaled, absv=absv, base=base)


def _vertices(u, v, depth, kinv):
    fxi, fyi, cxi, cyi = (F32(k) for k in kinv)
    u, v, depth = np.asarray(u, F32), np.asarray(v, F32), np.asarray(depth, F32)
    dx, dy = PATTERN[:, 0].astype(F32), PATTERN[:, 1].astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = ((u[:, None] + dx[None, :]) * fxi + cxi) * depth[:, None]
        y = ((v[:, None] + dy[None, :]) * fyi + cyi) * depth[:, None]
    z = np.broadcast_to(depth[:, None], x.shape)
    assert x.dtype == F32 and y.dtype == F32
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(F32)


def refresh_pc(active, marginalized, kinv):
    """active / marginalized: dicts of u, v, idepth, hdif, maxRelBaseline (+ color [n, 8] uint8 for the marginalized
    ones), in window / push order, either may be None.  Returns (xyz [n, 3] float32, rgb [n, 3] uint8)."""
    xyz, rgb = [np.zeros((0, 3), F32)], [np.zeros((0, 3), np.uint8)]
    if active is not None and len(active["u"]):
        keep, depth, _ = cloud_keep(active["idepth"], active["hdif"], active["maxRelBaseline"])
        xyz.append(_vertices(np.asarray(active["u"])[keep], np.asarray(active["v"])[keep], depth[keep], kinv))
        rgb.append(np.tile(np.array([[0, 0, 255]], np.uint8), (int(keep.sum()) * 8, 1)))  # the reference's `blue`
    if marginalized is not None and len(marginalized["u"]):
        keep, depth, _ = cloud_keep(marginalized["idepth"], marginalized["hdif"], marginalized["maxRelBaseline"])
        xyz.append(_vertices(np.asarray(marginalized["u"])[keep], np.asarray(marginalized["v"])[keep], depth[keep],
                             kinv))
        c = np.asarray(marginalized["color"], np.uint8)[keep].reshape(-1)
        rgb.append(np.stack([c, c, c], -1))
    return np.concatenate(xyz), np.concatenate(rgb)


def color_u8(color):
    """Vec3b(color[k], ...): float -> unsigned char, truncation toward zero."""
    return np.asarray(color, F32).astype(np.int32).astype(np.uint8)


def affine_factor(exp_newest, exp_f, a_newest, a_f):
    """refToFh[0] of AffLight::fromToVecExposure(newest, frame): exp(a_f - a_newest) * e_f / e_newest in double, the
    exposures being floats (both 1 when either is 0)."""
    eF, eT = float(F32(exp_newest)), float(F32(exp_f))
    if eF == 0 or eT == 0:
        eF = eT = 1.0
    return np.exp(float(a_f) - float(a_newest)) * eT / eF


def frame_scores(dist, kf_id, min_frame_age):
    """The distance score of every frame that passes the age test (None for the others)."""
    nF = len(kf_id)
    latest = int(kf_id[-1])
    out = []
    for f in range(nF):
        if kf_id[f] > latest - min_frame_age or kf_id[f] == 0:
            out.append(None)
            continue
        s = 0.0
        for t in range(nF):
            if kf_id[t] > latest - min_frame_age + 1 or t == f:
                continue
            s += 1 / (1e-5 + float(F32(dist[f, t])))
        s *= -float(np.sqrt(F32(dist[f, nF - 1])))
        out.append(s)
    return out


def frame_rule(n_in, n_out, aff0, dist, kf_id, P):
    """P: any object with minFrameAge, maxFrames, minFrames, minPointsRemaining, maxLogAffFacInWindow.  dist [nF, nF]
    float32, [h, t] the pair (host h, target t).  Returns (flagged [nF] uint8, why [nF] uint8)."""
    nF = len(kf_id)
    flagged, why = np.zeros(nF, np.uint8), np.zeros(nF, np.uint8)
    if P.minFrameAge > P.maxFrames:
        for i in range(P.maxFrames, nF):
            flagged[i - P.maxFrames] = 1
            why[i - P.maxFrames] |= WHY_AGE
        return flagged, why
    n = 0
    for f in range(nF):
        few = bool(F32(n_in[f]) < F32(P.minPointsRemaining) * F32(int(n_in[f]) + int(n_out[f])))
        aff = bool(np.abs(np.log(F32(aff0[f]))) > F32(P.maxLogAffFacInWindow))
        if not (few or aff):
            continue
        if nF - n > P.minFrames:
            flagged[f] = 1
            n += 1
            why[f] |= (WHY_POINTS if few else 0) | (WHY_AFFINE if aff else 0)
        else:
            why[f] |= WHY_BLOCKED
    if nF - n >= P.maxFrames:
        smallest, pick = 1.0, -1
        for f, s in enumerate(frame_scores(np.asarray(dist, F32).reshape(nF, nF), kf_id, P.minFrameAge)):
            if s is not None and s < smallest:
                smallest, pick = s, f
        if pick >= 0:  # the reference dereferences an empty toMarginalize otherwise; the library flags nothing
            flagged[pick] = 1
            why[pick] |= WHY_SCORE
    return flagged, why
