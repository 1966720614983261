"""The numpy statement of include/hs_flow.h's contract: the pyramid, the Scharr derivative and the per-point
Lucas-Kanade iteration of Initializer::FindMatches, in the header's order of operations.  Every float operation is a
rounded float32 operation (np.float32 scalars throughout), every sum over the window an exact integer sum, so the
kernels and this file agree bit for bit.  Besides (xy, status, err) it returns, per point, the exit reason of every
level and the number of iterations run."""
import numpy as np

F = np.float32
WIN = 15
PAD = 15
HALF = F(7.0)
MAX_LEVEL = 2
MAX_ITERS = 30
K5 = (1, 4, 6, 4, 1)
FLT_SCALE = F(1.0) / F(1 << 20)
FLT_EPSILON = F(np.finfo(np.float32).eps)
ERR_SCALE = F(1.0) / F(7200)
EPS2 = 0.01 * 0.01          # doubles

# exit reasons of a level; NOT_RUN marks a level the image does not have
CONVERGED, OSCILLATION, ITER_CAP, LEFT_IMAGE, MIN_EIG, PREV_OUTSIDE, ERR_OUTSIDE = range(7)
NOT_RUN = -1
REASONS = ("converged", "oscillation", "iteration cap", "left the image", "minEig/D", "previous window outside",
           "error window outside")


def refl(i, n):
    i = np.asarray(i)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def level_sizes(w, h):
    sizes = [(w, h)]
    while len(sizes) <= MAX_LEVEL:
        nw, nh = (sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2
        if nw <= WIN or nh <= WIN:
            break
        sizes.append((nw, nh))
    return sizes


def n_levels(w, h):
    return len(level_sizes(w, h))


def pyr_down(img):
    src = np.asarray(img, np.uint8).astype(np.int32)
    h, w = src.shape
    ow, oh = (w + 1) // 2, (h + 1) // 2
    xs, ys = 2 * np.arange(ow), 2 * np.arange(oh)
    hor = sum(K5[j] * src[:, refl(xs + j - 2, w)] for j in range(5))
    ver = sum(K5[j] * hor[refl(ys + j - 2, h), :] for j in range(5))
    return ((ver + 128) >> 8).astype(np.uint8)


def scharr(img):
    """(h, w, 2) int16: (dx, dy)"""
    I = np.asarray(img, np.uint8).astype(np.int32)
    h, w = I.shape
    y, x = np.arange(h), np.arange(w)
    up, dn = I[refl(y - 1, h)], I[refl(y + 1, h)]
    t0 = 3 * (up + dn) + 10 * I
    t1 = dn - up
    xl, xr = refl(x - 1, w), refl(x + 1, w)
    dx = t0[:, xr] - t0[:, xl]
    dy = 3 * (t1[:, xr] + t1[:, xl]) + 10 * t1
    return np.stack([dx, dy], axis=-1).astype(np.int16)


def pyramid(img):
    """the levels that exist, level 0 first"""
    img = np.ascontiguousarray(img, np.uint8)
    levels = [img]
    for _ in level_sizes(img.shape[1], img.shape[0])[1:]:
        levels.append(pyr_down(levels[-1]))
    return levels


def _pad_img(a):
    return np.pad(a, PAD, mode="reflect").astype(np.int64)


def _pad_deriv(d):
    return np.pad(d, ((PAD, PAD), (PAD, PAD), (0, 0))).astype(np.int64)


def _inside(px, py, w, h):
    return bool(px >= -WIN and px < w and py >= -WIN and py < h)   # NaN fails every comparison


def _weights(px, py):
    """after _inside: (ipx, ipy, (iw00, iw01, iw10, iw11))"""
    ipx, ipy = int(np.floor(px)), int(np.floor(py))
    a, b = F(px - F(ipx)), F(py - F(ipy))
    one = F(1)
    iw00 = int(np.rint(F(F(F(one - a) * F(one - b)) * F(16384))))
    iw01 = int(np.rint(F(F(a * F(one - b)) * F(16384))))
    iw10 = int(np.rint(F(F(F(one - a) * b) * F(16384))))
    return ipx, ipy, (iw00, iw01, iw10, 16384 - iw00 - iw01 - iw10)


def _bilinear(pad, ipx, ipy, iw):
    """sum of taps * iw over the 15 x 15 window whose top-left tap is (ipx, ipy); pad: (H+30, W+30[, c]) int64"""
    t = pad[ipy + PAD:ipy + PAD + WIN + 1, ipx + PAD:ipx + PAD + WIN + 1]
    return iw[0] * t[:-1, :-1] + iw[1] * t[:-1, 1:] + iw[2] * t[1:, :-1] + iw[3] * t[1:, 1:]


def _f32(int_sum):
    return F(int(int_sum))     # exact in double, rounded once to float32


def calc(prev, nxt, prev_xy, init_xy=None):
    """One calcOpticalFlowPyrLK(prev, nxt, prev_xy) by the contract.  Returns dict(xy (n, 2) f32, status (n,) u8,
    err (n,) f32, reasons (n, 3) i8 indexed by level, iters (n,) i32)."""
    prev_l, next_l = pyramid(prev), pyramid(nxt)
    assert prev_l[0].shape == next_l[0].shape
    L = len(prev_l)
    I_pad = [_pad_img(a) for a in prev_l]
    D_pad = [_pad_deriv(scharr(a)) for a in prev_l]
    J_pad = [_pad_img(a) for a in next_l]
    prev_xy = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
    n = len(prev_xy)
    if init_xy is not None:
        init_xy = np.ascontiguousarray(init_xy, np.float32).reshape(-1, 2)
        assert len(init_xy) == n
    xy = np.zeros((n, 2), np.float32)
    status = np.ones(n, np.uint8)
    err = np.zeros(n, np.float32)
    reasons = np.full((n, MAX_LEVEL + 1), NOT_RUN, np.int8)
    iters = np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for i in range(n):
            ox = oy = F(0)
            for l in range(L - 1, -1, -1):
                h, w = prev_l[l].shape
                s = F(1.0 / (1 << l))
                px, py = F(prev_xy[i, 0] * s), F(prev_xy[i, 1] * s)
                if l == L - 1:
                    gx, gy = (F(init_xy[i, 0] * s), F(init_xy[i, 1] * s)) if init_xy is not None else (px, py)
                else:
                    gx, gy = F(ox * F(2)), F(oy * F(2))
                ox, oy = gx, gy
                px, py = F(px - HALF), F(py - HALF)
                if not _inside(px, py, w, h):
                    reasons[i, l] = PREV_OUTSIDE
                    if l == 0:
                        status[i] = 0
                    continue
                ipx, ipy, iw = _weights(px, py)
                Iw = (_bilinear(I_pad[l], ipx, ipy, iw) + 256) >> 9
                dw = (_bilinear(D_pad[l], ipx, ipy, iw) + 8192) >> 14
                Ix, Iy = dw[..., 0], dw[..., 1]
                A11 = F(_f32(np.sum(Ix * Ix)) * FLT_SCALE)
                A12 = F(_f32(np.sum(Ix * Iy)) * FLT_SCALE)
                A22 = F(_f32(np.sum(Iy * Iy)) * FLT_SCALE)
                D = F(F(A11 * A22) - F(A12 * A12))
                dA = F(A11 - A22)
                root = F(np.sqrt(F(F(dA * dA) + F(F(F(4) * A12) * A12))))
                min_eig = F(F(F(A22 + A11) - root) / F(450))
                if float(min_eig) < 1e-4 or D < FLT_EPSILON:
                    reasons[i, l] = MIN_EIG
                    if l == 0:
                        status[i] = 0
                    continue
                D = F(F(1) / D)
                qx, qy = F(gx - HALF), F(gy - HALF)
                pdx = pdy = F(0)
                reason = ITER_CAP
                for j in range(MAX_ITERS):
                    if not _inside(qx, qy, w, h):
                        reason = LEFT_IMAGE
                        if l == 0:
                            status[i] = 0
                        break
                    iqx, iqy, jw = _weights(qx, qy)
                    diff = ((_bilinear(J_pad[l], iqx, iqy, jw) + 256) >> 9) - Iw
                    b1 = F(_f32(np.sum(diff * Ix)) * FLT_SCALE)
                    b2 = F(_f32(np.sum(diff * Iy)) * FLT_SCALE)
                    dx = F(F(F(A12 * b2) - F(A22 * b1)) * D)
                    dy = F(F(F(A12 * b1) - F(A11 * b2)) * D)
                    iters[i] += 1
                    qx, qy = F(qx + dx), F(qy + dy)
                    ox, oy = F(qx + HALF), F(qy + HALF)
                    if float(dx) * float(dx) + float(dy) * float(dy) <= EPS2:
                        reason = CONVERGED
                        break
                    if j > 0 and abs(float(F(dx + pdx))) < 0.01 and abs(float(F(dy + pdy))) < 0.01:
                        ox, oy = F(ox - F(dx * F(0.5))), F(oy - F(dy * F(0.5)))
                        reason = OSCILLATION
                        break
                    pdx, pdy = dx, dy
                reasons[i, l] = reason
                if l == 0 and status[i]:
                    ex, ey = F(ox - HALF), F(oy - HALF)
                    if not _inside(ex, ey, w, h):
                        status[i] = 0
                        reasons[i, l] = ERR_OUTSIDE
                    else:
                        iex, iey, ew = _weights(ex, ey)
                        ad = np.abs(((_bilinear(J_pad[l], iex, iey, ew) + 256) >> 9) - Iw)
                        err[i] = F(_f32(np.sum(ad)) * ERR_SCALE)
            xy[i] = (ox, oy)
    return dict(xy=xy, status=status, err=err, reasons=reasons, iters=iters)


def mean_flow(prev_xy, xy, good):
    """Initializer::ComputeMeanOpticalFlow with its accumulate-into-int: acc = (int)(acc + norm) over the good
    points, divided by (float)count (NaN for no good point: 0 / 0.f)."""
    acc, cnt = 0, 0
    for p, q, g in zip(np.asarray(prev_xy, np.float32), np.asarray(xy, np.float32), good):
        if not g:
            continue
        dx, dy = float(F(p[0] - q[0])), float(F(p[1] - q[1]))
        acc = int(F(acc) + F(np.sqrt(dx * dx + dy * dy)))
        cnt += 1
    with np.errstate(all="ignore"):
        return F(F(acc) / F(cnt))


class Matcher:
    """Initializer::FindMatches' bookkeeping over calc(): the chain the device context is compared with."""

    def __init__(self, img, xy):
        self.img = np.ascontiguousarray(img, np.uint8)
        self.first_xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2).copy()
        self.prev_xy = self.first_xy.copy()
        self.xy = self.first_xy.copy()
        self.last = None

    def track(self, img, max_l1_error):
        r = calc(self.img, img, self.xy, self.xy)
        self.prev_xy, self.xy = self.xy, r["xy"]
        self.img = np.ascontiguousarray(img, np.uint8)
        r["good"] = ((r["status"] != 0) & (r["err"] < F(max_l1_error))).astype(np.uint8)
        r["prev_xy"] = self.prev_xy
        self.last = r
        return int(r["good"].sum())
