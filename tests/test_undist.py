"""The host tables of include/hs_undist.h (hs_undist_make_remap, hs_undist_make_photometric) against the numpy
restatement tests/undist_ref.py.  No GPU: the table builders are host code.

Bars.  Pinhole and RadTan use only exactly rounded operations (+ - * / and conversions), so their K and maps are
bit-exact.  Atan, EquiDistant and KannalaBrandt call atan / tan / atan2, where libm and numpy may differ by 1 ulp:
K stays exact (useK does not touch the distortion), map entries agree within 8 * 2^-23 * max(w_in, h_in) pixels
(about six float roundings plus two libm calls of <= 1 ulp each, at coordinate magnitude), and the valid / -1
classification is identical except where the reference's coordinate lies within that bound of a threshold of the
validity pass; at most 0.1 % of the entries may be excused that way."""
import numpy as np
import pytest

import undist_ref
from undist_cases import CASES, gamma_G, lib_calib, random_vignette, ref_remap


@pytest.fixture(scope="module")
def refs():
    """Reference tables, computed once per case and shared."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ref_remap(name, raw_coords=True)
        return cache[name]
    return get


@pytest.mark.parametrize("name", ["kitti", "euroc", "small_crop", "small_usek"])
def test_make_remap_exact(name, refs):
    from hslam_amd.undistort import make_remap
    K, rx, ry = make_remap(lib_calib(name))
    Kr, rxr, ryr, _, _ = refs(name)
    assert np.array_equal(K, Kr), (K, Kr)
    assert np.array_equal(rx, rxr)
    assert np.array_equal(ry, ryr)


@pytest.mark.parametrize("name", ["tum", "equi", "kb"])
def test_make_remap_tolerance(name, refs):
    from hslam_amd.undistort import make_remap
    c = CASES[name]
    K, rx, ry = make_remap(lib_calib(name))
    Kr, rxr, ryr, x0, y0 = refs(name)
    assert np.array_equal(K, Kr), (K, Kr)
    bound = 8 * 2.0 ** -23 * max(c["w_in"], c["h_in"])
    wlim, hlim = c["w_in"] - 1, c["h_in"] - 1
    # the validity pass tests x against 0 and w_in - 1, y against 0, h_in - 1 (the nudge) and w_in - 1 (as written)
    x64, y64 = x0.astype(np.float64), y0.astype(np.float64)
    near = (np.minimum(np.abs(x64), np.abs(x64 - wlim)) <= bound) | \
           (np.minimum(np.minimum(np.abs(y64), np.abs(y64 - hlim)), np.abs(y64 - wlim)) <= bound)
    valid, valid_r = rx != -1, rxr != -1
    assert np.array_equal(valid, ry != -1) and np.array_equal(valid_r, ryr != -1)
    both = valid & valid_r
    err = np.where(both, np.maximum(np.abs(rx.astype(np.float64) - rxr), np.abs(ry.astype(np.float64) - ryr)), 0.0)
    off = (valid != valid_r) | (err > bound)
    print(f"{name}: bound {bound:.3e} px, max map difference {err.max():.3e} px, class differences "
          f"{int((valid != valid_r).sum())}, entries near a threshold {int(near.sum())}, excused {int(off.sum())}")
    assert not np.any(off & ~near), f"{int((off & ~near).sum())} entries differ away from every threshold"
    assert off.sum() <= 0.001 * off.size


def test_calib_struct_matches_c_layout(tmp_path):
    """The ctypes mirror of hs_undist_calib has the C struct's size and field offsets (compiled here with gcc)."""
    import ctypes
    import os
    import subprocess
    from hslam_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hs_undist.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(hs_undist_calib), offsetof(hs_undist_calib, K_in),'
                   ' offsetof(hs_undist_calib, dist), offsetof(hs_undist_calib, desired_K));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)],
                   check=True)
    sizes = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    c = _lib.hs_undist_calib
    assert sizes == [ctypes.sizeof(c), c.K_in.offset, c.dist.offset, c.desired_K.offset]


def test_make_remap_rejects():
    from hslam_amd._lib import HsError
    from hslam_amd.undistort import make_calib, make_remap
    with pytest.raises(HsError, match="equal"):
        make_remap(make_calib("Pinhole", 64, 48, 32, 24, (40, 40, 31.5, 23.5), process="none"))
    with pytest.raises(HsError, match="size"):
        make_remap(make_calib("Pinhole", 64, 0, 32, 24, (40, 40, 31.5, 23.5), process="crop"))
    # a camera centre far outside the image: no border ever maps inside, the crop loop runs out of iterations
    with pytest.raises(HsError, match="500"):
        make_remap(make_calib("Pinhole", 64, 48, 32, 24, (40, 40, -5000.0, 23.5), process="crop"))


def test_photometric_tables_exact():
    from hslam_amd.undistort import make_photometric
    G, vig = gamma_G(), random_vignette((64, 96))
    Binv, B, vinv = make_photometric(G, vig)
    Br, BBr, vr = undist_ref.make_photometric(G, vig)
    assert np.array_equal(Binv, Br) and np.array_equal(B, BBr) and np.array_equal(vinv, vr)
    assert Binv[0] == 0 and Binv[255] == 255 and B[255] == 255 and np.all(np.diff(B) >= 0)
    assert B[1] == 0 and Binv[1] > 1   # no segment s >= 1 brackets 1: the loop assigns nothing, the entry is 0
    # no G: identity both ways; no vignette: none
    Binv, B, vinv = make_photometric(None, None)
    assert np.array_equal(Binv, np.arange(256, dtype=np.float32)) and np.array_equal(B, Binv) and vinv is None
    Br, BBr, _ = undist_ref.make_photometric(None, None)
    assert np.array_equal(Binv, Br) and np.array_equal(B, BBr)


def test_photometric_rejects_bad_G():
    from hslam_amd._lib import HsError
    from hslam_amd.undistort import make_photometric
    G = gamma_G()
    with pytest.raises(HsError, match="256"):
        make_photometric(G[:255], None)
    flat = G.copy()
    flat[100] = flat[99]
    with pytest.raises(HsError, match="increasing"):
        make_photometric(flat, None)
    down = G.copy()
    down[200] = down[199] - 1
    with pytest.raises(HsError, match="increasing"):
        make_photometric(down, None)


def test_reference_inputs_exercise_the_border(refs):
    """The reference alone: the inputs the GPU tests use reach the paths they are meant to reach."""
    c = CASES["small_usek"]
    _, rx, ry, _, _ = refs("small_usek")
    invalid = (rx == -1).mean()
    deep = int(((rx != -1) & (ry >= c["h_in"] - 1)).sum())
    print(f"small_usek: {100 * invalid:.1f} % invalid, {deep} valid entries with remap_y >= h_in - 1")
    assert 0.05 <= invalid <= 0.25
    assert deep >= 1   # valid by the as-written test against w_in, bottom taps outside: the border path is live
    c = CASES["euroc"]
    _, rx, ry, _, _ = refs("euroc")
    print(f"euroc: {int((rx == -1).sum())} invalid, {int(((rx != -1) & (ry >= c['h_in'] - 1)).sum())} valid entries "
          f"with remap_y >= h_in - 1")
