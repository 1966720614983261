"""include/hs_image.h without a device: the argument checks of hs_image_create come before any device call, and the
ctypes signatures of the new entries load."""
import ctypes as C

import pytest

ENTRIES = ("hs_image_create", "hs_image_destroy", "hs_image_set_u8", "hs_image_set_raw", "hs_image_get",
           "hs_image_last_stats", "hs_tracker_set_frame_image", "hs_tracer_set_frame_image",
           "hs_tracer_set_host_image_from", "hs_selector_make_maps_image", "hs_extractor_extract_image",
           "hs_flow_track_image", "hs_image_to_ba")


def test_signatures_load():
    from hslam_amd._lib import SIGNATURES, load
    lib = load()
    for name in ENTRIES:
        assert name in SIGNATURES, name
        fn = getattr(lib, name)
        assert list(fn.argtypes) == SIGNATURES[name][0] and fn.restype == SIGNATURES[name][1], name


def test_header_declares_every_entry():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "hs_image.h")).read()
    for name in ENTRIES:
        assert name + "(" in text, name


@pytest.mark.parametrize("args, word", [
    ((0, 64, 3), "side"),        # a side < 1
    ((64, 0, 3), "side"),
    ((-5, 64, 1), "side"),
    ((64, 48, 0), "n_levels"),   # n_levels outside what hs_tracker_create accepts
    ((64, 48, 7), "n_levels"),
    ((64, 16, 6), "small"),      # 16 >> 5 = 0: the top level would be empty
])
def test_create_rejects_before_any_device_call(args, word):
    """HS_ERR_INVALID with a message; an invalid device id shows that no device call was reached."""
    from hslam_amd._lib import load
    lib = load()
    h = C.c_void_p(1)
    assert lib.hs_image_create(C.byref(h), 4096, *args) == -1
    assert not h.value
    assert word in lib.hs_last_error().decode()


def test_create_null_out():
    from hslam_amd._lib import load
    lib = load()
    assert lib.hs_image_create(None, 4096, 64, 48, 3) == -1
    assert "null" in lib.hs_last_error().decode()


def test_null_image_arguments():
    from hslam_amd._lib import load
    lib = load()
    lib.hs_image_destroy(None)
    ms = C.c_double()
    for rc in (lib.hs_image_set_u8(None, None, None), lib.hs_image_set_raw(None, None),
               lib.hs_image_get(None, 0, None, None, None), lib.hs_image_last_stats(None, C.byref(ms)),
               lib.hs_tracker_set_frame_image(None, None, 1.0), lib.hs_tracer_set_frame_image(None, None),
               lib.hs_tracer_set_host_image_from(None, 0, None), lib.hs_extractor_extract_image(None, None, None, None),
               lib.hs_flow_track_image(None, None, 7.0, None), lib.hs_image_to_ba(None, None, 0),
               lib.hs_selector_make_maps_image(None, 0, None, 100.0, 1, 1.0, None, None)):
        assert rc == -1
