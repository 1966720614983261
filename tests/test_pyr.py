"""Frame::CreateDirPyrs (Src/Frame.cpp:104-181): the oracle restatement, the device kernels and the contexts' raw
frame entries.  Bar: bit-exact (the pyramid is elementwise fp32 arithmetic in the reference's operation order)."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def raw():
    from hslam_amd.scene import make_track_scene
    s = make_track_scene(n_points=400, width=320, height=240, n_levels=4,
                         K=np.array([[128.0, 0, 159.5], [0, 127.2, 119.5], [0, 0, 1.0]]))
    return s


def test_oracle_matches_scene_pyramid(raw):
    """The oracle restatement against the numpy generator the scenes use (hslam_amd.scene.make_dir_pyramid)."""
    from hslam_amd.scene import make_dir_pyramid
    from oracle_ffi import dir_pyramid
    img = raw.new_pyr[0][..., 0]
    po, go = dir_pyramid(img, 4)
    pn = make_dir_pyramid(img, 4)
    for l in range(4):
        assert np.array_equal(po[l], pn[l]), l
        g = po[l][..., 1] ** 2 + po[l][..., 2] ** 2
        assert np.array_equal(go[l], g.astype(np.float32)), l


def test_oracle_nonfinite_gradients_are_zero():
    from oracle_ffi import dir_pyramid
    img = np.full((16, 24), 7.0, np.float32)
    img[5, 6] = np.inf
    p, _ = dir_pyramid(img, 2)
    assert np.all(np.isfinite(p[0][..., 1:])) and np.isinf(p[0][5, 6, 0])


# (width, height, levels): the smallest shapes at which the build's 32 x 32 tiling can go wrong
TILE_SHAPES = [(4, 4, 1),      # the smallest legal frame: one partial tile, no fold
               (5, 7, 2),      # odd sides in one partial tile: the unused last column and row
               (33, 31, 3),    # a second tile that is one pixel wide, and a bottom row cut one short
               (64, 64, 6),    # HS_MAX_LEVELS: the fold down to one pixel per tile, a 2 x 2 top level
               (97, 65, 6)]    # partial tiles at every level, top level 3 x 2


def tile_images():
    """(name, image, levels) of the small cases: seeded random floats in [0, 255], and the non-finite pixel."""
    out = []
    for w, h, levels in TILE_SHAPES:
        rng = np.random.default_rng(1000 * w + h)
        out.append((f"{w}x{h}x{levels}", rng.uniform(0.0, 255.0, size=(h, w)).astype(np.float32), levels))
    img = np.full((16, 24), 7.0, np.float32)
    img[5, 6] = np.inf
    out.append(("24x16x2 inf", img, 2))
    return out


def test_oracle_small_shapes():
    """The oracle half of the small device cases: level sizes, zero first / last rows, the non-finite rule."""
    from oracle_ffi import dir_pyramid
    for name, img, levels in tile_images():
        h, w = img.shape
        p, g = dir_pyramid(img, levels)
        assert np.array_equal(p[0][..., 0], img), name
        for l in range(levels):
            assert p[l].shape == (h >> l, w >> l, 3) and g[l].shape == (h >> l, w >> l), (name, l)
            assert not p[l][0, :, 1:].any() and not p[l][-1, :, 1:].any(), (name, l)
            assert np.all(np.isfinite(p[l][..., 1:])) and np.all(np.isfinite(g[l])), (name, l)
            if l > 0:
                s = p[l - 1][..., 0]
                hl, wl = h >> l, w >> l
                q = np.float32(0.25) * (((s[0:2 * hl:2, 0:2 * wl:2] + s[0:2 * hl:2, 1:2 * wl:2]) +
                                         s[1:2 * hl:2, 0:2 * wl:2]) + s[1:2 * hl:2, 1:2 * wl:2])
                assert np.array_equal(p[l][..., 0], q), (name, l)


@pytest.mark.gpu
def test_device_pyramid_bit_exact(raw):
    from hslam_amd.pyr import dir_pyramid as dev
    from oracle_ffi import dir_pyramid
    cases = [("new", raw.new_pyr[0][..., 0], 4), ("ref", raw.ref_pyr[0][..., 0], 4)] + tile_images()
    for name, img, levels in cases:
        pg, gg = dev(img, levels)
        po, go = dir_pyramid(img, levels)
        for l in range(levels):
            # all three texel lanes and absSquaredGrad, bitwise (an inf intensity compares equal to itself)
            assert pg[l].tobytes() == po[l].tobytes(), (name, l)
            assert gg[l].tobytes() == go[l].tobytes(), (name, l)


@pytest.mark.gpu
def test_tracker_raw_frame_matches_host_pyramid(raw):
    from hslam_amd.track import CoarseTracker
    a = CoarseTracker(raw.width, raw.height, raw.K4, raw.n_levels)
    a.set_scene(raw)
    b = CoarseTracker(raw.width, raw.height, raw.K4, raw.n_levels)
    b.setCoarseTrackingRef(raw.ref_pyr, raw.ref_exposure, raw.ref_aff, raw.pt_u, raw.pt_v, raw.pt_idepth, raw.pt_hdi)
    b.setNewFrameRaw(raw.new_pyr[0][..., 0], raw.new_exposure)
    for lvl in range(raw.n_levels):
        ra, _, _, na = a.calcRes(lvl, raw.T_true, raw.aff_true, 20.0)
        rb, _, _, nb = b.calcRes(lvl, raw.T_true, raw.aff_true, 20.0)
        assert na == nb and np.array_equal(ra, rb), lvl


@pytest.mark.gpu
def test_tracer_raw_frame_matches_host_image():
    from hslam_amd.scene import make_trace_scene
    from hslam_amd.trace import ImmatureTracer
    s = make_trace_scene(n_points=500, n_hosts=4, width=320, height=240, seed=9)
    a = ImmatureTracer(s.width, s.height, s.n_points)
    a.set_scene(s)
    b = ImmatureTracer(s.width, s.height, s.n_points)
    for i, im in enumerate(s.host_imgs):
        b.set_host_image(i, im)
    b.add_points(s.pt_host, s.pt_u, s.pt_v)
    b.set_frame_raw(s.new_img[..., 0])
    assert np.array_equal(a.traceNewCoarse(s.KRKi, s.Kt, s.aff), b.traceNewCoarse(s.KRKi, s.Kt, s.aff))
    pa, pb = a.points(), b.points()
    for k in pa:
        assert np.array_equal(pa[k], pb[k], equal_nan=True), k
