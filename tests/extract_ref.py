"""numpy restatement of the contract in include/hs_extract.h (FeatureDetector::ExtractFeatures with UseFAST = false and
DoSubPix = false): the thing the device is held to.  Integer steps are exact; float steps are float32 with every
operation rounded, in the header's order.

OpenCV is not available where this project is built and tested, so the blur weights and fastAtan2 below restate OpenCV's
published behaviour (its 8-bit fixed-point GaussianBlur and its scalar fastAtan2) and are not pinned against it.

The descriptor goes through cos / sin in double, where the device's math library and numpy's may differ in the last
place; ``descriptors`` therefore flags as ambiguous every bit one of whose four tap coordinates lies within TIE_EPS of
a rounding tie, the only place such a difference can change a bit."""
import numpy as np

BORDER = 19
HALF_PATCH = 15
PATTERN_MAX = 13
TIE_EPS = 1e-4
F = np.float32


def blur_weights():
    """The 7 taps for sigma 2 as 8-bit fixed point: normalised Gaussian in double times 256, rounded from the outer
    tap inward with the rounding error carried into the next tap, mirrored; the centre is what is left of 256."""
    g = np.exp(-((np.arange(7) - 3.0) ** 2) / (2.0 * 2.0 * 2.0))
    g = g / g.sum() * 256.0
    w = np.zeros(7, np.int64)
    err = 0.0
    for k in range(3):
        v = g[k] + err
        w[k] = int(np.rint(v))
        err = v - w[k]
        w[6 - k] = w[k]
    w[3] = 256 - w.sum()
    return w


def reflect101(i, n):
    i = np.asarray(i)
    return np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def blur(img):
    """cv::GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101) on u8 as fixed point: (H, W) uint8 -> (H, W) uint8."""
    src = np.asarray(img, np.uint8).astype(np.int64)
    H, W = src.shape
    w = blur_weights()
    cols = reflect101(np.arange(-3, W + 3), W)
    rows = reflect101(np.arange(-3, H + 3), H)
    h = sum(w[k] * src[:, cols[k:k + W]] for k in range(7))
    assert h.max() < 65536
    v = sum(w[k] * h[rows[k:k + H], :] for k in range(7))
    return ((v + 32768) >> 16).astype(np.uint8)


def umax():
    """InitUmax's rule for half patch 15: rounded half widths up to 45 degrees, mirrored about the diagonal beyond."""
    hp = HALF_PATCH
    um = np.zeros(hp + 2, np.int64)
    vmax = int(np.floor(F(hp) * np.sqrt(F(2)) / F(2) + F(1)))
    vmin = int(np.ceil(F(hp) * np.sqrt(F(2)) / F(2)))
    for v in range(vmax + 1):
        um[v] = int(np.rint(np.sqrt(float(hp * hp - v * v))))
    v0 = 0
    for v in range(hp, vmin - 1, -1):
        while um[v0] == um[v0 + 1]:
            v0 += 1
        um[v] = v0
        v0 += 1
    return um[: hp + 1]


def keys(selection_map):
    """mvKeys[i].pt: (n, 2) float32 (x, y) of the nonzero pixels of the interior, in raster order."""
    m = np.asarray(selection_map)
    H, W = m.shape
    ys, xs = np.nonzero(m[BORDER:H - BORDER, BORDER:W - BORDER] != 0)   # row-major: raster order
    return np.stack([xs + BORDER, ys + BORDER], 1).astype(np.float32)


def fast_atan2(y, x):
    """cv::fastAtan2's scalar form in float32, degrees; y, x arrays (or scalars)."""
    y = np.atleast_1d(np.asarray(y, F))
    x = np.atleast_1d(np.asarray(x, F))
    scale = F(180.0 / np.pi)
    p1, p3, p5, p7 = (F(0.9997878412794807) * scale, F(-0.3258083974640975) * scale, F(0.1555786518463281) * scale,
                      F(-0.04432655554792128) * scale)
    eps = F(2.220446049250313e-16)
    ax, ay = np.abs(x), np.abs(y)
    wide = ax >= ay
    num = np.where(wide, ay, ax)
    den = np.where(wide, ax, ay) + eps
    c = (num / den).astype(F)
    c2 = c * c
    poly = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(wide, poly, F(90) - poly).astype(F)
    a = np.where(x < 0, F(180) - a, a).astype(F)
    a = np.where(y < 0, F(360) - a, a).astype(F)
    assert a.dtype == F and c2.dtype == F and poly.dtype == F
    return a


def moments(img, xy):
    """(m10, m01) int64 of IC_Angle's disc around every key of the unblurred image."""
    img = np.asarray(img, np.uint8).astype(np.int64)
    um = umax()
    du = np.concatenate([np.arange(-um[abs(v)], um[abs(v)] + 1) for v in range(-HALF_PATCH, HALF_PATCH + 1)])
    dv = np.concatenate([np.full(2 * um[abs(v)] + 1, v) for v in range(-HALF_PATCH, HALF_PATCH + 1)])
    x = xy[:, 0].astype(np.int64)[:, None]
    y = xy[:, 1].astype(np.int64)[:, None]
    I = img[y + dv[None, :], x + du[None, :]]
    m10, m01 = (I * du[None, :]).sum(1), (I * dv[None, :]).sum(1)
    assert np.all(np.abs(m10) < 2 ** 24) and np.all(np.abs(m01) < 2 ** 24)
    return m10, m01


def angles(img, xy):
    if len(xy) == 0:
        return np.zeros(0, F)
    m10, m01 = moments(img, xy)
    return fast_atan2(m01.astype(F), m10.astype(F))


def tap_offsets(angle, pattern):
    """For angles (n,) float32 degrees and a (256, 2, 2) pattern: the unrounded float32 tap coordinates
    (tx, ty), each (n, 256, 2)."""
    pat = np.asarray(pattern, np.int8).reshape(256, 2, 2).astype(F)
    rad = np.asarray(angle, F) * F(np.pi / 180.0)
    a = np.cos(rad.astype(np.float64)).astype(F)[:, None, None]
    b = np.sin(rad.astype(np.float64)).astype(F)[:, None, None]
    px, py = pat[None, :, :, 0], pat[None, :, :, 1]
    ty = (px * b).astype(F) + (py * a).astype(F)
    tx = (px * a).astype(F) - (py * b).astype(F)
    assert tx.dtype == F and ty.dtype == F
    return tx, ty


def ambiguous_bits(tx, ty):
    """(n, 256) bool: a coordinate of either tap within TIE_EPS of k + 0.5."""
    def near_tie(t):
        t = t.astype(np.float64)
        return np.abs(t - np.floor(t) - 0.5) < TIE_EPS
    return (near_tie(tx) | near_tie(ty)).any(axis=2)


def descriptors(blurred, xy, angle, pattern):
    """(desc (n, 32) uint8, ambiguous (n, 256) bool)."""
    n = len(xy)
    if n == 0:
        return np.zeros((0, 32), np.uint8), np.zeros((0, 256), bool)
    b = np.asarray(blurred, np.uint8)
    tx, ty = tap_offsets(angle, pattern)
    xo = np.rint(tx).astype(np.int64)   # half to even
    yo = np.rint(ty).astype(np.int64)
    x = xy[:, 0].astype(np.int64)[:, None, None]
    y = xy[:, 1].astype(np.int64)[:, None, None]
    val = b[y + yo, x + xo]             # an index outside the image would raise or wrap: the bounds rule is checked
    assert (y + yo).min() >= 0 and (x + xo).min() >= 0
    bits = val[:, :, 0] < val[:, :, 1]
    desc = np.packbits(bits, axis=1, bitorder="little")
    return desc, ambiguous_bits(tx, ty)


def extract(selection_map, img8, pattern):
    """One ExtractFeatures: dict(xy, angle, desc, ambiguous, blurred)."""
    xy = keys(selection_map)
    blurred = blur(img8)
    ang = angles(img8, xy)
    desc, amb = descriptors(blurred, xy, ang, pattern)
    return dict(xy=xy, angle=ang, desc=desc, ambiguous=amb, blurred=blurred)


def unpack_bits(desc):
    return np.unpackbits(np.asarray(desc, np.uint8), axis=1, bitorder="little").astype(bool)
