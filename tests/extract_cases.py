"""Inputs the extraction tests share (tests/test_extract.py on the host, tests/test_gpu_extract.py on the device), and
the reference's result for them, computed once per process and never modified."""
import functools

import numpy as np

import extract_ref

W, H = 101, 67          # odd, no multiple of the blur tile, more than one tile each way
MAX_AMBIGUOUS = 0.005   # the share of descriptor bits the reference may flag (a condition on the inputs)


def random_pattern(seed=7):
    """A sampling pattern as H-SLAM would pass its own: (256, 2, 2) int8, every entry within +-13."""
    return np.random.default_rng(seed).integers(-13, 14, size=(256, 2, 2), dtype=np.int8)


def random_image(w=W, h=H, seed=1):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8)


def random_map(w=W, h=H, seed=2, density=0.25):
    """A selection map with PixelSelector's values (0, 1, 2, 4) all over the image, the border included."""
    rng = np.random.default_rng(seed)
    m = rng.choice(np.array([1, 2, 4], np.float32), size=(h, w))
    m[rng.random((h, w)) >= density] = 0
    return m


def ramp_image(sx, sy, w=W, h=H):
    """Brightness rising along (sx, sy): the intensity centroid of every disc falls in that quadrant."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.rint(128 + sx * 1.0 * (x - w / 2) + sy * 0.7 * (y - h / 2)).astype(np.uint8)


def sparse_map(w, h, step=11):
    m = np.zeros((h, w), np.float32)
    m.ravel()[::step] = 1
    return m


def vga_image():
    from hslam_amd.scene import make_select_frames
    return make_select_frames(1, width=640, height=480)[0]


@functools.lru_cache(maxsize=None)
def descriptor_case():
    """(map, image, pattern, reference result) of the random-image descriptor test."""
    m, img, pat = random_map(), random_image(), random_pattern()
    return m, img, pat, extract_ref.extract(m, img, pat)


def ambiguous_share(ref):
    return float(ref["ambiguous"].mean()) if ref["ambiguous"].size else 0.0
