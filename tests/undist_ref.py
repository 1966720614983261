"""numpy restatement of include/hs_undist.h, float32 operation by operation: the test reference of the host tables
(GeometricUndistorter's remap and K, PhotometricUndistorter's Binv / B / vignette) and of the kernel's contract
(photometric pass over the whole input, then cv::remap INTER_LINEAR as documented arithmetic: the two-pass form).
A double literal in the reference's float expressions makes that subexpression float64 here too."""
import numpy as np

f32, f64 = np.float32, np.float64
PINHOLE, ATAN, RADTAN, EQUIDISTANT, KANNALABRANDT = range(5)
MODELS = {"Pinhole": PINHOLE, "Atan": ATAN, "RadTan": RADTAN, "EquiDistant": EQUIDISTANT,
          "KannalaBrandt": KANNALABRANDT}


def distort(model, ic, K, x, y):
    """distortCoordinates: float32 arrays of output-image coordinates -> input-image coordinates."""
    fx, fy, cx, cy = (f32(v) for v in ic[:4])
    ofx, ofy, ocx, ocy = (f32(v) for v in K)
    d = [f32(v) for v in ic[4:8]]
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    ix = (x - ocx) / ofx
    iy = (y - ocy) / ofy
    with np.errstate(all="ignore"):
        if model == PINHOLE:
            return fx * ix + cx, fy * iy + cy
        if model == ATAN:
            dist = d[0]
            d2t = f32(2) * np.tan(dist / f32(2))
            r = np.sqrt(ix * ix + iy * iy)
            fac = np.where((r == 0) | (dist == 0), f32(1), np.arctan(r * d2t) / (dist * r)).astype(f32)
            return fx * fac * ix + cx, fy * fac * iy + cy
        if model == RADTAN:
            k1, k2, r1, r2 = d
            mx2, my2, mxy = ix * ix, iy * iy, ix * iy
            rho2 = mx2 + my2
            rad = k1 * rho2 + k2 * rho2 * rho2
            D = lambda a: a.astype(f64)
            xd = (D(ix + ix * rad) + 2.0 * f64(r1) * D(mxy) + f64(r2) * (D(rho2) + 2.0 * D(mx2))).astype(f32)
            yd = (D(iy + iy * rad) + 2.0 * f64(r2) * D(mxy) + f64(r1) * (D(rho2) + 2.0 * D(my2))).astype(f32)
            return fx * xd + cx, fy * yd + cy
        if model == EQUIDISTANT:
            k1, k2, k3, k4 = d
            r = np.sqrt(ix * ix + iy * iy)
            th = np.arctan(r)
            th2 = th * th
            th4 = th2 * th2
            th6 = th4 * th2
            th8 = th4 * th4
            thd = th * (f32(1) + k1 * th2 + k2 * th4 + k3 * th6 + k4 * th8)
            scaling = np.where(r.astype(f64) > 1e-8, thd / r, f32(1)).astype(f32)
            return fx * ix * scaling + cx, fy * iy * scaling + cy
        assert model == KANNALABRANDT
        k0, k1, k2, k3 = d
        s = np.sqrt(ix * ix + iy * iy)
        th = np.arctan2(s, f32(1))
        th2 = th * th
        th3 = th2 * th
        th5 = th3 * th2
        th7 = th5 * th2
        th9 = th7 * th2
        r = th + k0 * th3 + k1 * th5 + k2 * th7 + k3 * th9
        small = s.astype(f64) < 1e-6
        ox = np.where(small, fx * ix + cx, (r / s) * fx * ix + cx).astype(f32)
        oy = np.where(small, fy * iy + cy, (r / s) * fy * iy + cy).astype(f32)
        return ox, oy


def _optimal_k_crop(model, ic, w, h, w_in, h_in):
    K = [1.0, 1.0, 0.0, 0.0]
    wlim, hlim = f32(w_in - 1), f32(h_in - 1)
    samples = (np.arange(100000, dtype=f32) - f32(50000)) / f32(10000)
    zeros = np.zeros(100000, f32)

    def first_last(vals, lim):
        # the reference's scan: min is assigned while it is still 0, max at every sample inside
        inside = samples[(vals > 0) & (vals < lim)]
        nz = inside[inside != 0]
        return (nz[0] if nz.size else f32(0)), (inside[-1] if inside.size else f32(0))

    minX, maxX = first_last(distort(model, ic, K, samples, zeros)[0], wlim)
    minY, maxY = first_last(distort(model, ic, K, zeros, samples)[1], hlim)
    minX, maxX, minY, maxY = (f32(f64(v) * 1.01) for v in (minX, maxX, minY, maxY))

    ys, xs = np.arange(h, dtype=f32), np.arange(w, dtype=f32)
    oob = [True] * 4
    iteration = 0
    while any(oob):
        by = (minY + (maxY - minY) * ys / (f32(h) - f32(1))).astype(f32)
        lx = distort(model, ic, K, np.full(h, minX, f32), by)[0]
        rx = distort(model, ic, K, np.full(h, maxX, f32), by)[0]
        oobL = bool(np.any(~((lx > 0) & (lx < wlim))))
        oobR = bool(np.any(~((rx > 0) & (rx < wlim))))
        bx = (minX + (maxX - minX) * xs / (f32(w) - f32(1))).astype(f32)
        ty = distort(model, ic, K, bx, np.full(w, minY, f32))[1]
        by2 = distort(model, ic, K, bx, np.full(w, maxY, f32))[1]
        oobT = bool(np.any(~((ty > 0) & (ty < hlim))))
        oobB = bool(np.any(~((by2 > 0) & (by2 < hlim))))
        if (oobL or oobR) and (oobT or oobB):
            if (maxX - minX) > (maxY - minY):
                oobB = oobT = False
            else:
                oobL = oobR = False
        if oobL:
            minX = f32(f64(minX) * 0.995)
        if oobR:
            maxX = f32(f64(maxX) * 0.995)
        if oobT:
            minY = f32(f64(minY) * 0.995)
        if oobB:
            maxY = f32(f64(maxY) * 0.995)
        oob = [oobL, oobR, oobT, oobB]
        iteration += 1
        if iteration > 500:
            raise ValueError("crop: no output K found in 500 iterations")
    K[0] = f64((f32(w) - f32(1)) / (maxX - minX))
    K[1] = f64((f32(h) - f32(1)) / (maxY - minY))
    K[2] = f64(-minX) * K[0]
    K[3] = f64(-minY) * K[1]
    return K


def make_remap(model, w_in, h_in, w_out, h_out, K_in, dist, process, desired_K=None, raw_coords=False):
    """(K float32 (4,), remap_x, remap_y (h_out, w_out) float32).  raw_coords: also return the coordinates before
    the validity pass (the tolerance tests look at distances to its thresholds)."""
    model = MODELS.get(model, model)
    Kl = [float(v) for v in K_in]
    if Kl[2] < 1 and Kl[3] < 1:
        Kl = [Kl[0] * w_in, Kl[1] * h_in, Kl[2] * w_in - 0.5, Kl[3] * h_in - 0.5]
    d = [float(v) for v in np.atleast_1d(dist)][:4]
    d += [0.0] * (4 - len(d))
    if model == PINHOLE:
        d = [0.0] * 4
    elif model == ATAN:
        d = [d[0], 0.0, 0.0, 0.0]
    ic = Kl + d
    if process == "crop":
        K = _optimal_k_crop(model, ic, w_out, h_out, w_in, h_in)
    elif process == "none":
        assert (w_in, h_in) == (w_out, h_out)
        K = list(Kl)
    else:
        assert process == "useK"
        K = [desired_K[0] * w_out, desired_K[1] * h_out, desired_K[2] * w_out - 0.5, desired_K[3] * h_out - 0.5]
    gx, gy = np.meshgrid(np.arange(w_out, dtype=f32), np.arange(h_out, dtype=f32))
    x0, y0 = distort(model, ic, K, gx, gy)
    wlim, hlim = f32(w_in - 1), f32(h_in - 1)
    ix, iy = x0.copy(), y0.copy()
    ix = np.where(ix == 0, f32(0.001), ix)
    iy = np.where(iy == 0, f32(0.001), iy)
    ix = np.where(ix == wlim, f32(w_in - 1.001), ix)
    ix = np.where(iy == hlim, f32(h_in - 1.001), ix)       # as written in the reference: ix, from hOrg
    ok = (ix > 0) & (iy > 0) & (ix < wlim) & (iy < wlim)   # as written: iy against wOrg
    rx = np.where(ok, ix, f32(-1)).astype(f32)
    ry = np.where(ok, iy, f32(-1)).astype(f32)
    Kf = np.array(K, f64).astype(f32)
    return (Kf, rx, ry, x0, y0) if raw_coords else (Kf, rx, ry)


def make_photometric(G=None, vignette=None):
    """(Binv, B, vignette_inv or None): the normalised response, UpdateGamma's inverse, max / v."""
    if G is None:
        Binv = np.arange(256, dtype=f32)
    else:
        g = np.asarray(G, f32)
        assert g.shape == (256,) and np.all(g[1:] > g[:-1])
        Binv = (255.0 * (g - g[0]).astype(f64) / f64(g[255] - g[0])).astype(f32)
    B = np.zeros(256, f32)
    for i in range(1, 255):
        hit = np.nonzero((Binv[1:255] <= f32(i)) & (Binv[2:256] >= f32(i)))[0]
        if hit.size:
            s = int(hit[0]) + 1
            B[i] = f32(s) + (f32(i) - Binv[s]) / (Binv[s + 1] - Binv[s])
    B[0], B[255] = 0, 255
    vinv = None
    if vignette is not None:
        v = np.asarray(vignette, np.uint16).astype(f32)
        vinv = (v.max() / v).astype(f32)
    return Binv, B, vinv


def sat8(a):
    """cv::saturate_cast<uchar>(float): round half to even, clamped."""
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def tap_classes(raw_shape, rx, ry):
    """Per output pixel, how many of its four taps lie inside the input (4 = inner, 1..3 partly, 0 wholly outside)."""
    h_in, w_in = raw_shape
    sx = np.rint(np.asarray(rx, f32) * f32(32)).astype(np.int32)
    sy = np.rint(np.asarray(ry, f32) * f32(32)).astype(np.int32)
    ix, iy = sx >> 5, sy >> 5
    n = np.zeros(ix.shape, np.int32)
    for dy in (0, 1):
        for dx in (0, 1):
            n += ((ix + dx >= 0) & (ix + dx < w_in) & (iy + dy >= 0) & (iy + dy < h_in)).astype(np.int32)
    return n


def undistort(raw, rx, ry, Binv=None, B=None, vinv=None, passthrough=False):
    """(fImg float32, img8 uint8) of a raw u8 frame.  B is given whenever photometric tables are in use."""
    raw = np.asarray(raw, np.uint8)
    h_in, w_in = raw.shape
    # pass 1: the photometric correction of the whole input
    S = Binv[raw] if Binv is not None else raw.astype(f32)
    if vinv is not None:
        S = (S * np.asarray(vinv, f32).reshape(raw.shape)).astype(f32)
    S = S.astype(f32)
    if passthrough:
        f = S
    else:
        # pass 2: remap, INTER_LINEAR, constant 0 border
        sx = np.rint(np.asarray(rx, f32) * f32(32)).astype(np.int32)
        sy = np.rint(np.asarray(ry, f32) * f32(32)).astype(np.int32)
        ix, iy = sx >> 5, sy >> 5
        fx = (sx & 31).astype(f32) * f32(1.0 / 32)
        fy = (sy & 31).astype(f32) * f32(1.0 / 32)
        one = f32(1)
        w0, w1, w2, w3 = (one - fy) * (one - fx), (one - fy) * fx, fy * (one - fx), fy * fx

        def tap(yy, xx):
            inside = (xx >= 0) & (xx < w_in) & (yy >= 0) & (yy < h_in)
            v = S[np.clip(yy, 0, h_in - 1), np.clip(xx, 0, w_in - 1)]
            return np.where(inside, v, f32(0)).astype(f32)

        f = tap(iy, ix) * w0 + tap(iy, ix + 1) * w1 + tap(iy + 1, ix) * w2 + tap(iy + 1, ix + 1) * w3
        f = f.astype(f32)
    img8 = sat8(B[sat8(f)]) if B is not None else sat8(f)
    return f, img8
