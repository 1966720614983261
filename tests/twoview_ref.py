"""The contract of include/hs_twoview.h in numpy: what the two-view fit's kernels are held to.

Every step is the arithmetic the header states, in the same order and the same number formats: fp32 where the header
says fp32 (numpy float32 arrays, no fused multiply-add), fp64 elsewhere, the fixed-order sum `sum256`, and the one-sided
cyclic Jacobi of h-slam_amd/csrc/hs_jacobi.h restated over a batch (`jacobi_cols`).  OpenCV is not a dependency, so
parity with cv::SVD is not pinned; tests/test_twoview.py holds the Jacobi to numpy.linalg.svd instead.

`fit` also returns what the tests need to know about the model itself: the winners' margins over the runners-up and,
per match, whether a tested quantity lies within a relative 1e-4 of its threshold (`amb_*`)."""
import numpy as np

f32, f64 = np.float32, np.float64
MAX_SWEEPS = 16
TOL = 2.0 ** -50
AMB = 1e-4
TH_H, TH_F, TH_SCORE = f32(5.991), f32(3.841), f32(5.991)
COS_MIN = 0.99998
# cosParallax is tested 2e-5 below 1, where fp32 steps are 2^-24: a relative 1e-4 band around 0.99998 would span 1600 of
# them and excuse every low-parallax match, and a relative 1e-4 of the quantity really tested (1 - cos against 2e-5) is
# below one step.  The band is 4 steps: narrower than the literal reading, so it excuses fewer matches.
AMB_COS = 4 * 2.0 ** -24
TH2 = f32(4.0)


# ---- the shared pieces

def sum256(x):
    """The header's fixed-order fp64 sum over the last axis of x (..., n)."""
    x = np.asarray(x, f64)
    n = x.shape[-1]
    rows = (n + 255) // 256
    pad = np.zeros(x.shape[:-1] + (rows * 256,), f64)
    pad[..., :n] = x
    m = pad.reshape(x.shape[:-1] + (rows, 256))
    part = np.zeros(x.shape[:-1] + (256,), f64)
    for r in range(rows):
        part = part + m[..., r, :]
    s = 128
    while s > 0:
        part = part[..., :s] + part[..., s:2 * s]
        s >>= 1
    return part[..., 0]


def jacobi_cols(A):
    """hs::jacobi_cols over a batch: A (B, M, N) float64 -> (A_out, V), A_in @ V = A_out with orthogonal columns."""
    A = np.array(A, f64)
    B, M, N = A.shape
    V = np.broadcast_to(np.eye(N), (B, N, N)).copy()
    with np.errstate(all="ignore"):
        for _ in range(MAX_SWEEPS):
            rotated = False
            for p in range(N - 1):
                for q in range(p + 1, N):
                    al = np.zeros(B)
                    be = np.zeros(B)
                    ga = np.zeros(B)
                    for i in range(M):
                        a, b = A[:, i, p], A[:, i, q]
                        al = al + a * a
                        be = be + b * b
                        ga = ga + a * b
                    skip = (ga == 0.0) | (np.abs(ga) <= TOL * np.sqrt(al * be))
                    if skip.all():
                        continue
                    rotated = True
                    zeta = (be - al) / (2.0 * ga)
                    t = np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    c = 1.0 / np.sqrt(1.0 + t * t)
                    s = c * t
                    c = np.where(skip, 1.0, c)[:, None]
                    s = np.where(skip, 0.0, s)[:, None]
                    keep = skip[:, None]
                    for X in (A, V):
                        a, b = X[:, :, p].copy(), X[:, :, q].copy()
                        X[:, :, p] = np.where(keep, a, c * a - s * b)
                        X[:, :, q] = np.where(keep, b, s * a + c * b)
            if not rotated:
                break
    return A, V


def col_norm2(A):
    n2 = np.zeros((A.shape[0], A.shape[2]))
    for i in range(A.shape[1]):
        n2 = n2 + A[:, i, :] * A[:, i, :]
    return n2


def null_vector(A):
    """hs::jacobi_null_vector over a batch (B, M, N) -> (B, N)."""
    Ao, V = jacobi_cols(A)
    j = np.argmin(col_norm2(Ao), axis=1)
    return V[np.arange(len(V)), :, j]


def mul3(a, b):
    return (a[..., :, 0:1] * b[..., 0:1, :] + a[..., :, 1:2] * b[..., 1:2, :]) + a[..., :, 2:3] * b[..., 2:3, :]


def det3(m):
    m = m.reshape(m.shape[:-2] + (9,))
    return (m[..., 0] * (m[..., 4] * m[..., 8] - m[..., 5] * m[..., 7])
            - m[..., 1] * (m[..., 3] * m[..., 8] - m[..., 5] * m[..., 6])
            + m[..., 2] * (m[..., 3] * m[..., 7] - m[..., 4] * m[..., 6]))


def inv3(M):
    m = M.reshape(M.shape[:-2] + (9,))
    d = det3(M)
    o = np.stack([(m[..., 4] * m[..., 8] - m[..., 5] * m[..., 7]) / d, (m[..., 2] * m[..., 7] - m[..., 1] * m[..., 8]) / d,
                  (m[..., 1] * m[..., 5] - m[..., 2] * m[..., 4]) / d, (m[..., 5] * m[..., 6] - m[..., 3] * m[..., 8]) / d,
                  (m[..., 0] * m[..., 8] - m[..., 2] * m[..., 6]) / d, (m[..., 2] * m[..., 3] - m[..., 0] * m[..., 5]) / d,
                  (m[..., 3] * m[..., 7] - m[..., 4] * m[..., 6]) / d, (m[..., 1] * m[..., 6] - m[..., 0] * m[..., 7]) / d,
                  (m[..., 0] * m[..., 4] - m[..., 1] * m[..., 3]) / d], -1)
    return o.reshape(M.shape)


def svd3(A, rank3):
    """hs::jacobi_svd3 on one 3 x 3 matrix -> U, w, Vt."""
    Ao, V = jacobi_cols(np.asarray(A, f64)[None])
    Ao, V = Ao[0], V[0]
    n2 = col_norm2(Ao[None])[0]
    o = [0, 1, 2]
    for i in range(1, 3):
        j = i
        while j > 0 and n2[o[j]] > n2[o[j - 1]]:
            o[j], o[j - 1] = o[j - 1], o[j]
            j -= 1
    w = np.sqrt(n2[o])
    Vt = V[:, o].T.copy()
    with np.errstate(all="ignore"):
        U = Ao[:, o] / w[None, :]
    if not rank3:
        U[0, 2] = U[1, 0] * U[2, 1] - U[2, 0] * U[1, 1]
        U[1, 2] = U[2, 0] * U[0, 1] - U[0, 0] * U[2, 1]
        U[2, 2] = U[0, 0] * U[1, 1] - U[1, 0] * U[0, 1]
    return U, w, Vt


# ---- Normalize (:1090-1136)

def normalize(xy):
    """(meanX, meanY, sX, sY) in float32."""
    xy = np.asarray(xy, f32)
    n = f64(len(xy))
    out = []
    for c in (0, 1):
        x = xy[:, c]
        mean = f32(sum256(x.astype(f64)) / n)
        dev = f32(sum256(np.abs(x - mean).astype(f64)) / n)
        with np.errstate(all="ignore"):
            out.append((mean, f32(1.0 / f64(dev))))
    return out[0][0], out[1][0], out[0][1], out[1][1]


# ---- hypotheses (:557-633)

def design_matrices(xy1, xy2, sets):
    """The fp32 A of ComputeH21 (ns, 16, 9) and ComputeF21 (ns, 8, 9) widened to float64, and (T1, T2) as fp32 entries."""
    n1, n2 = normalize(xy1), normalize(xy2)
    xy1, xy2 = np.asarray(xy1, f32), np.asarray(xy2, f32)
    sets = np.asarray(sets)
    u1 = (xy1[sets, 0] - n1[0]) * n1[2]
    v1 = (xy1[sets, 1] - n1[1]) * n1[3]
    u2 = (xy2[sets, 0] - n2[0]) * n2[2]
    v2 = (xy2[sets, 1] - n2[1]) * n2[3]
    ns = len(sets)
    z, one = np.zeros_like(u1), np.ones_like(u1)
    r0 = np.stack([z, z, z, -u1, -v1, -one, v2 * u1, v2 * v1, v2], -1)
    r1 = np.stack([u1, v1, one, z, z, z, -u2 * u1, -u2 * v1, -u2], -1)
    AH = np.stack([r0, r1], 2).reshape(ns, 16, 9).astype(f64)
    AF = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, one], -1).astype(f64)
    assert r0.dtype == f32 and AF.shape == (ns, 8, 9)
    return AH, AF, n1, n2


def t_matrix(nm):
    mx, my, sx, sy = nm
    return np.array([[sx, 0, -mx * sx], [0, sy, -my * sy], [0, 0, 1]], f32).astype(f64)


def hypotheses(xy1, xy2, sets, null=null_vector):
    """H21, H12, F21: (ns, 3, 3) float32 each."""
    AH, AF, n1, n2 = design_matrices(xy1, xy2, sets)
    ns = len(AH)
    T1, T2 = t_matrix(n1), t_matrix(n2)
    with np.errstate(all="ignore"):
        T2inv = np.array([[1.0 / T2[0, 0], 0, -T2[0, 2] / T2[0, 0]], [0, 1.0 / T2[1, 1], -T2[1, 2] / T2[1, 1]], [0, 0, 1]])
        Hn = null(AH).reshape(ns, 3, 3)
        H21 = mul3(mul3(T2inv[None], Hn), T1[None])
        H12 = inv3(H21)
        Fpre = null(AF).reshape(ns, 3, 3)
        B, V = jacobi_cols(Fpre)
        drop = np.argmin(col_norm2(B), axis=1)
        Fn = np.zeros((ns, 3, 3))
        for k in range(3):
            term = B[:, :, k, None] * V[:, None, :, k]
            Fn = np.where((drop != k)[:, None, None], Fn + term, Fn)
        F21 = mul3(mul3(T2.T.copy()[None], Fn), T1[None])
        return H21.astype(f32), H12.astype(f32), F21.astype(f32)


# ---- scores (:635-809)

def _recip(x):
    with np.errstate(all="ignore"):
        return (1.0 / x.astype(f64)).astype(f32)


def contributions_h(H21, H12, xy1, xy2, status):
    """Per (hypothesis, match): c1, c2 (float32, 0 where nothing is added), bIn, and the chi values."""
    H = np.asarray(H21, f32).reshape(-1, 9)[:, :, None]
    Hi = np.asarray(H12, f32).reshape(-1, 9)[:, :, None]
    u1, v1, u2, v2 = (np.asarray(a, f32)[None, :] for a in (xy1[:, 0], xy1[:, 1], xy2[:, 0], xy2[:, 1]))
    with np.errstate(all="ignore"):
        w2 = _recip((Hi[:, 6] * u2 + Hi[:, 7] * v2) + Hi[:, 8])
        a = ((Hi[:, 0] * u2 + Hi[:, 1] * v2) + Hi[:, 2]) * w2
        b = ((Hi[:, 3] * u2 + Hi[:, 4] * v2) + Hi[:, 5]) * w2
        chi1 = (u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)
        w1 = _recip((H[:, 6] * u1 + H[:, 7] * v1) + H[:, 8])
        a = ((H[:, 0] * u1 + H[:, 1] * v1) + H[:, 2]) * w1
        b = ((H[:, 3] * u1 + H[:, 4] * v1) + H[:, 5]) * w1
        chi2 = (u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)
        return _finish_contrib(chi1, chi2, TH_H, TH_H, status)


def contributions_f(F21, xy1, xy2, status):
    F = np.asarray(F21, f32).reshape(-1, 9)[:, :, None]
    u1, v1, u2, v2 = (np.asarray(a, f32)[None, :] for a in (xy1[:, 0], xy1[:, 1], xy2[:, 0], xy2[:, 1]))
    with np.errstate(all="ignore"):
        a2 = (F[:, 0] * u1 + F[:, 1] * v1) + F[:, 2]
        b2 = (F[:, 3] * u1 + F[:, 4] * v1) + F[:, 5]
        c2 = (F[:, 6] * u1 + F[:, 7] * v1) + F[:, 8]
        num2 = (a2 * u2 + b2 * v2) + c2
        chi1 = num2 * num2 / (a2 * a2 + b2 * b2)
        a1 = (F[:, 0] * u2 + F[:, 3] * v2) + F[:, 6]
        b1 = (F[:, 1] * u2 + F[:, 4] * v2) + F[:, 7]
        c1 = (F[:, 2] * u2 + F[:, 5] * v2) + F[:, 8]
        num1 = (a1 * u1 + b1 * v1) + c1
        chi2 = num1 * num1 / (a1 * a1 + b1 * b1)
        return _finish_contrib(chi1, chi2, TH_F, TH_SCORE, status)


def _finish_contrib(chi1, chi2, th, th_score, status):
    assert chi1.dtype == f32 and chi2.dtype == f32
    live = (np.asarray(status) != 0)[None, :]
    out1, out2 = chi1 > th, chi2 > th
    c1 = np.where(out1 | ~live, f32(0), th_score - chi1).astype(f32)
    c2 = np.where(out2 | ~live, f32(0), th_score - chi2).astype(f32)
    inl = live & ~out1 & ~out2
    amb = live & ((np.abs(chi1 - th) <= AMB * th) | (np.abs(chi2 - th) <= AMB * th))
    return c1, c2, inl, amb


def scores_of(c1, c2):
    """(float32) sum256 with each match's two contributions added in order into the partial."""
    B, n = c1.shape
    rows = (n + 255) // 256
    p1 = np.zeros((B, rows * 256))
    p2 = np.zeros((B, rows * 256))
    p1[:, :n], p2[:, :n] = c1, c2
    p1, p2 = p1.reshape(B, rows, 256), p2.reshape(B, rows, 256)
    part = np.zeros((B, 256))
    for r in range(rows):
        part = part + p1[:, r]
        part = part + p2[:, r]
    s = 128
    while s > 0:
        part = part[:, :s] + part[:, s:2 * s]
        s >>= 1
    return part[:, 0].astype(f32)


def winner(scores):
    """(best, its score, margin): the lowest index that attains the maximum of the scores above 0, -1 when none; the
    margin is (best - runner-up) / best (1 when there is no runner-up)."""
    v = np.where(scores > 0, scores, f32(0)).astype(f32)
    if not (v.max() > 0):
        return -1, f32(0), 1.0
    b = int(np.argmax(v))
    rest = np.delete(v, b)
    margin = 1.0 if len(rest) == 0 else float((f64(v[b]) - f64(rest.max())) / f64(v[b]))
    return b, v[b], margin


def score_models(H21, H12, F21, xy1, xy2, status):
    xy1, xy2 = np.asarray(xy1, f32), np.asarray(xy2, f32)
    o = {}
    for name, (c1, c2, inl, amb) in (("h", contributions_h(H21, H12, xy1, xy2, status)),
                                     ("f", contributions_f(F21, xy1, xy2, status))):
        sc = scores_of(c1, c2)
        b, s, margin = winner(sc)
        o["scores_" + name] = sc
        o["best_" + name], o["S" + name.upper()], o["margin_" + name] = b, s, margin
        o["inliers_" + name] = (inl[b] if b >= 0 else np.zeros(len(status), bool)).astype(np.uint8)
        o["amb_" + name] = amb[b] if b >= 0 else np.zeros(len(status), bool)
    return o


# ---- motion hypotheses (:811-1073, :1261-1281)

def k_matrix(K4):
    fx, fy, cx, cy = (f32(x) for x in K4)
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)


def motions_f(F21, K4):
    K = k_matrix(K4).astype(f64)
    E = mul3(mul3(K.T.copy(), np.asarray(F21, f32).astype(f64).reshape(3, 3)), K)
    U, w, Vt = svd3(E, False)
    t = U[:, 2].copy()
    t = t / np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    R1 = mul3(mul3(U, W), Vt)
    if det3(R1) < 0:
        R1 = -R1
    R2 = mul3(mul3(U, W.T.copy()), Vt)
    if det3(R2) < 0:
        R2 = -R2
    R = np.stack([R1, R2, R1, R2]).astype(f32)
    tt = np.stack([t, t, -t, -t]).astype(f32)
    return R, tt


def motions_h(H21, K4):
    """(R (8, 3, 3), t (8, 3)) float32, or None when the singular values are too close (:941)."""
    K = k_matrix(K4).astype(f64)
    Kinv = np.array([[1.0 / K[0, 0], 0, -K[0, 2] / K[0, 0]], [0, 1.0 / K[1, 1], -K[1, 2] / K[1, 1]], [0, 0, 1]])
    A = mul3(mul3(Kinv, np.asarray(H21, f32).astype(f64).reshape(3, 3)), K)
    U, w, Vt = svd3(A, True)
    s = det3(U) * det3(Vt)
    d1, d2, d3 = w
    with np.errstate(all="ignore"):
        if f64(f32(d1) / f32(d2)) < 1.00001 or f64(f32(d2) / f32(d3)) < 1.00001:
            return None
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1 = [aux1, aux1, -aux1, -aux1]
        x3 = [aux3, -aux3, aux3, -aux3]
        aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        stheta = [aux_st, -aux_st, -aux_st, aux_st]
        aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sphi = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        Rs, ts = [], []
        for h in range(8):
            i = h & 3
            Rp = np.eye(3)
            if h < 4:
                Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ctheta, -stheta[i], stheta[i], ctheta
                tp = np.array([x1[i] * (d1 - d3), 0.0, -x3[i] * (d1 - d3)])
            else:
                Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cphi, sphi[i], -1.0, sphi[i], -cphi
                tp = np.array([x1[i] * (d1 + d3), 0.0, x3[i] * (d1 + d3)])
            R = s * mul3(mul3(U, Rp), Vt)
            t = (U[:, 0] * tp[0] + U[:, 1] * tp[1]) + U[:, 2] * tp[2]
            t = t / np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
            Rs.append(R)
            ts.append(t)
        return np.stack(Rs).astype(f32), np.stack(ts).astype(f32)


# ---- CheckRT (:1138-1259)

def order_statistic(values, k):
    return np.sort(np.asarray(values, f32), kind="stable")[k]


def parallax_of(cos_values):
    if len(cos_values) == 0:
        return f32(0)
    c = order_statistic(cos_values, min(50, len(cos_values) - 1))
    ac = f32(np.arccos(f64(c)))
    return f32(f64(ac * f32(180.0)) / np.pi)


def check_rt(R, t, xy1, xy2, inliers, K4):
    """One motion hypothesis over the matches with inliers != 0: dict(n_good, parallax, good, passed, cos, p3d (fp32),
    p3d64 (the fp64 x3D before its rounding), amb)."""
    xy1, xy2 = np.asarray(xy1, f32), np.asarray(xy2, f32)
    R = np.asarray(R, f32).reshape(3, 3)
    t = np.asarray(t, f32).reshape(3)
    K = k_matrix(K4)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    n = len(xy1)
    idx = np.flatnonzero(np.asarray(inliers) != 0)
    m = len(idx)
    Rt = np.concatenate([R, t[:, None]], 1)
    P1 = np.concatenate([K, np.zeros((3, 1), f32)], 1)
    P2 = ((K[:, 0:1] * Rt[0:1, :] + K[:, 1:2] * Rt[1:2, :]) + K[:, 2:3] * Rt[2:3, :]).astype(f32)
    assert P2.dtype == f32
    k = np.concatenate([xy1[idx], xy2[idx]], 1)
    A = np.stack([k[:, 0:1] * P1[2][None] - P1[0][None], k[:, 1:2] * P1[2][None] - P1[1][None],
                  k[:, 2:3] * P2[2][None] - P2[0][None], k[:, 3:4] * P2[2][None] - P2[1][None]], 1)
    assert A.dtype == f32 and A.shape == (m, 4, 4)
    o = dict(good=np.zeros(n, np.uint8), passed=np.zeros(n, np.uint8), cos=np.zeros(n, f32), p3d=np.zeros((n, 3), f32),
             p3d64=np.zeros((n, 3)), amb=np.zeros(n, bool))
    if m == 0:
        o.update(n_good=0, parallax=f32(0))
        return o
    with np.errstate(all="ignore"):
        v = null_vector(A.astype(f64))
        x64 = v[:, :3] / v[:, 3:4]
        p = x64.astype(f32)
        X, Y, Z = p[:, 0], p[:, 1], p[:, 2]
        fin = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
        O2 = -((R[0] * t[0] + R[1] * t[1]) + R[2] * t[2])
        assert O2.dtype == f32
        n2 = p - O2[None]
        pd, nd = p.astype(f64), n2.astype(f64)
        dist1 = np.sqrt((pd[:, 0] * pd[:, 0] + pd[:, 1] * pd[:, 1]) + pd[:, 2] * pd[:, 2]).astype(f32)
        dist2 = np.sqrt((nd[:, 0] * nd[:, 0] + nd[:, 1] * nd[:, 1]) + nd[:, 2] * nd[:, 2]).astype(f32)
        dot = (pd[:, 0] * nd[:, 0] + pd[:, 1] * nd[:, 1]) + pd[:, 2] * nd[:, 2]
        cosP = (dot / (dist1 * dist2).astype(f64)).astype(f32)
        lowpar = cosP.astype(f64) < COS_MIN
        X2 = ((R[0, 0] * X + R[0, 1] * Y) + R[0, 2] * Z) + t[0]
        Y2 = ((R[1, 0] * X + R[1, 1] * Y) + R[1, 2] * Z) + t[1]
        Z2 = ((R[2, 0] * X + R[2, 1] * Y) + R[2, 2] * Z) + t[2]
        invZ1, invZ2 = _recip(Z), _recip(Z2)
        im1x, im1y = fx * X * invZ1 + cx, fy * Y * invZ1 + cy
        e1 = (im1x - k[:, 0]) * (im1x - k[:, 0]) + (im1y - k[:, 1]) * (im1y - k[:, 1])
        im2x, im2y = fx * X2 * invZ2 + cx, fy * Y2 * invZ2 + cy
        e2 = (im2x - k[:, 2]) * (im2x - k[:, 2]) + (im2y - k[:, 3]) * (im2y - k[:, 3])
        assert e1.dtype == f32 and e2.dtype == f32 and Z2.dtype == f32
        passed = fin & ~((Z <= 0) & lowpar) & ~((Z2 <= 0) & lowpar) & ~(e1 > TH2) & ~(e2 > TH2)
        amb = ((np.abs(cosP.astype(f64) - COS_MIN) <= AMB_COS) | (np.abs(Z) <= AMB * dist1)
               | (np.abs(Z2) <= AMB * dist2) | (np.abs(e1 - TH2) <= AMB * TH2) | (np.abs(e2 - TH2) <= AMB * TH2) | ~fin)
    o["passed"][idx] = passed
    o["good"][idx] = passed & lowpar
    o["cos"][idx] = np.where(passed, cosP, f32(0))
    o["p3d"][idx] = np.where(passed[:, None], p, f32(0))
    o["p3d64"][idx] = np.where(passed[:, None], x64, 0.0)
    o["amb"][idx] = amb
    o["n_good"] = int(passed.sum())
    o["parallax"] = parallax_of(cosP[passed])
    return o


# ---- the decision (:840-913, :1032-1072): the reference's control flow, branch by branch

def rule_f(n_good, parallax, N, min_parallax=1.0, min_tri=50):
    """(ok, why, best)."""
    max_good = max(n_good[:4])
    n_min_good = max(int(0.9 * N), min_tri)
    nsimilar = sum(1 for g in n_good[:4] if g > 0.7 * max_good)
    if max_good < n_min_good or nsimilar > 1:
        return 0, 3, -1
    for i in range(4):
        if max_good == n_good[i]:
            return (1, 0, i) if parallax[i] > f32(min_parallax) else (0, 4, i)
    return 0, 3, -1


def rule_h(n_good, parallax, N, min_parallax=1.0, min_tri=50):
    best_good, second, best_idx, best_par = 0, 0, -1, f32(-1)
    for i in range(8):
        if n_good[i] > best_good:
            second, best_good, best_idx, best_par = best_good, n_good[i], i, parallax[i]
        elif n_good[i] > second:
            second = n_good[i]
    if not (second < 0.75 * best_good and best_good > min_tri and best_good > 0.9 * N):
        return 0, 3, best_idx
    return (1, 0, best_idx) if best_par >= f32(min_parallax) else (0, 4, best_idx)


# ---- the whole fit

def fit(xy1, xy2, status, sets, K4):
    xy1, xy2 = np.asarray(xy1, f32), np.asarray(xy2, f32)
    status = np.asarray(status, np.uint8)
    n = len(xy1)
    H21, H12, F21 = hypotheses(xy1, xy2, sets)
    o = score_models(H21, H12, F21, xy1, xy2, status)
    o.update(H21=H21, H12=H12, F21=F21, ok=0, why=0, model=-1, n_rt=0, best_rt=-1, n_good=0, parallax=f32(0),
             n_triangulated=0, median_depth=f32(0), R=np.zeros((3, 3), f32), t=np.zeros(3, f32), n_inliers=0,
             triangulated=np.zeros(n, np.uint8), p3d=np.zeros((n, 3), f32), rt=[], amb_rt=np.zeros(n, bool))
    SH, SF = o["SH"], o["SF"]
    if SH == 0 and SF == 0:
        o["why"] = 1
        return o
    with np.errstate(all="ignore"):
        RH = f32(SH) / (f32(SH) + f32(SF))
    model = 0 if f64(RH) > 0.40 else 1
    o["model"] = model
    inl = o["inliers_f"] if model else o["inliers_h"]
    o["n_inliers"] = int(inl.sum())
    mot = motions_f(F21[o["best_f"]], K4) if model else motions_h(H21[o["best_h"]], K4)
    if mot is None:
        o["why"] = 2
        return o
    R, t = mot
    o["R_all"], o["t_all"] = R, t
    o["n_rt"] = len(R)
    rt = [check_rt(R[h], t[h], xy1, xy2, inl, K4) for h in range(len(R))]
    o["rt"] = rt
    n_good = [r["n_good"] for r in rt]
    par = [r["parallax"] for r in rt]
    ok, why, best = (rule_f if model else rule_h)(n_good, par, o["n_inliers"])
    o["amb_rt"] = np.any([r["amb"] for r in rt], axis=0)
    o["n_good_all"], o["parallax_all"] = n_good, par
    o.update(best_rt=best, n_good=n_good[best] if best >= 0 else 0, parallax=par[best] if best >= 0 else f32(0))
    if ok:
        good = rt[best]["good"] != 0
        ntri = int(good.sum())
        if ntri == 0:
            ok, why = 0, 3
        else:
            z = rt[best]["p3d"][good, 2]
            med = order_statistic(z, (ntri - 1) // 2)
            o["median_depth"] = med
            o["n_triangulated"] = ntri
            o["triangulated"] = good.astype(np.uint8)
            o["p3d"] = np.where(good[:, None], rt[best]["p3d"] / med, f32(0)).astype(f32)
            o["R"], o["t"] = R[best], (t[best] / med).astype(f32)
    o["ok"], o["why"] = ok, why
    return o
