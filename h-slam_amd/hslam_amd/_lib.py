"""Loader of the product library ``h-slam_amd/lib/libhslam_amd.so`` (HIP, gfx950).

There is no CPU fallback: if the library is missing, or no HIP device is present
when a context is created, the call raises.  Build with ``make -C h-slam_amd/csrc``
(or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_ROOT, "lib", "libhslam_amd.so")
# experiment builds only (h-slam_amd/csrc/Makefile `variant`); unset, the in-tree product library is loaded
if os.environ.get("HSLAM_AMD_LIB"):
    LIB_PATH = os.path.abspath(os.environ["HSLAM_AMD_LIB"])

# data-contract structs (include/hs_types.h)


class hs_camera(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("n_levels", C.c_int), ("pad", C.c_int),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class hs_frame(C.Structure):
    _fields_ = [("worldToCam_evalPT", C.c_double * 7), ("state", C.c_double * 10), ("state_zero", C.c_double * 10),
                ("ab_exposure", C.c_float), ("frameEnergyTH", C.c_float), ("id", C.c_int), ("pad", C.c_int)]


class hs_points(C.Structure):
    _fields_ = [("n", C.c_int), ("host", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("idepth", C.c_void_p),
                ("idepth_zero", C.c_void_p), ("color", C.c_void_p), ("weights", C.c_void_p),
                ("has_depth_prior", C.c_void_p)]


class hs_residuals(C.Structure):
    _fields_ = [("n", C.c_int), ("point", C.c_void_p), ("target", C.c_void_p), ("state", C.c_void_p)]


class hs_params(C.Structure):
    _fields_ = [(n, C.c_float) for n in (
        "huberTH", "outlierTHSumComponent", "frameEnergyTHN", "frameEnergyTHFacMedian", "frameEnergyTHConstWeight",
        "overallEnergyTHWeight", "idepthFixPrior", "initialCalibHessian", "affineOptModeA", "affineOptModeB",
        "initialRotPrior", "initialTransPrior", "initialAffAPrior", "initialAffBPrior")] + [
        ("solverModeDelta", C.c_double), ("thOptIterations", C.c_float), ("coarseCutoffTH", C.c_float),
        ("minOptIterations", C.c_int), ("pad", C.c_int)] + [(n, C.c_float) for n in (
        "outlierTH", "maxPixSearch", "trace_slackInterval", "trace_stepsize", "trace_minImprovementFactor",
        "trace_GNThreshold", "trace_extraSlackOnTH")] + [
        ("minTraceTestRadius", C.c_int), ("trace_GNIterations", C.c_int),
        ("idepthFixPriorMargFac", C.c_float), ("margWeightFac", C.c_float),
        ("desiredPointDensity", C.c_float), ("minTraceQuality", C.c_float), ("minIdepthH_act", C.c_float),
        ("GNItsOnPointActivation", C.c_int), ("minGradHistCut", C.c_float), ("minGradHistAdd", C.c_float),
        ("gradDownweightPerLevel", C.c_float), ("selectDirectionDistribution", C.c_int)]


class hs_undist_calib(C.Structure):  # include/hs_undist.h
    _fields_ = [("model", C.c_int), ("w_in", C.c_int), ("h_in", C.c_int), ("w_out", C.c_int), ("h_out", C.c_int),
                ("process", C.c_int), ("K_in", C.c_double * 4), ("dist", C.c_double * 4),
                ("desired_K", C.c_double * 4)]


class hs_fast_params(C.Structure):  # include/hs_extract.h
    _fields_ = [("threshold", C.c_int), ("num_features", C.c_int), ("min_dist", C.c_int), ("tolerance", C.c_float)]


class hs_map_record(C.Structure):  # include/hs_map.h
    _fields_ = [("handle", C.c_int32), ("frame_id", C.c_int32), ("status", C.c_int32), ("numGoodResiduals", C.c_int32),
                ("u", C.c_float), ("v", C.c_float), ("idepth", C.c_float), ("idepth_zero", C.c_float),
                ("hdif", C.c_float), ("maxRelBaseline", C.c_float), ("color", C.c_uint8 * 8),
                ("reserved", C.c_uint8 * 16)]


class hs_frame_marg_params(C.Structure):  # include/hs_map.h
    _fields_ = [("minFrameAge", C.c_int), ("maxFrames", C.c_int), ("minFrames", C.c_int),
                ("minPointsRemaining", C.c_float), ("maxLogAffFacInWindow", C.c_float)]


# exported symbols of include/hs_ba.h (argument types)
VP, I, D = C.c_void_p, C.c_int, C.c_double
SIGNATURES = {
    "hs_params_default": ([VP], I),
    "hs_last_error": ([], C.c_char_p),
    "hs_create": ([VP, VP, I], I),
    "hs_destroy": ([VP], None),
    "hs_ba_set_window": ([VP, VP, I, VP, VP, VP, VP], I),
    "hs_ba_linearize": ([VP, I, VP], I),
    "hs_ba_solve_system": ([VP, I, VP], I),
    "hs_ba_do_step": ([VP, VP], I),
    "hs_ba_optimize": ([VP, I, I, VP, VP], I),
    "hs_ba_iterate": ([VP, I, I, VP], I),
    "hs_ba_fix_linearization": ([VP, VP, VP, VP, VP, VP], I),
    "hs_ba_calc_energies": ([VP, VP, VP], I),
    "hs_ba_get_system": ([VP, I, VP, VP], I),
    "hs_ba_get_residuals": ([VP] * 7, I),
    "hs_ba_get_points": ([VP] * 5, I),
    "hs_ba_get_frames": ([VP] * 5, I),
    "hs_ba_set_marginal_prior": ([VP, VP, VP], I),
    "hs_ba_marginalize_points": ([VP, I, VP, VP, VP], I),
    "hs_ba_marginalize_frame": ([VP, I, VP, VP], I),
    "hs_ba_get_timings": ([VP, VP], I),
    "hs_ba_time_linearize": ([VP, I, VP], I),
    "hs_ba_get_partition": ([VP, VP], I),
    "hs_ba_reserve": ([VP, VP, I], I),
    "hs_ba_insert_frame": ([VP, VP, VP], I),
    "hs_ba_set_frame_image": ([VP, I, VP], I),
    "hs_ba_set_frame_image_raw": ([VP, I, VP], I),
    "hs_ba_set_frame_image_device": ([VP, I, VP], I),
    "hs_ba_insert_points": ([VP, VP, VP, VP, VP], I),
    "hs_ba_insert_residuals": ([VP, I, VP, VP, VP], I),
    "hs_ba_add_residuals_to_newest": ([VP, VP], I),
    "hs_ba_drop_residuals": ([VP, I, VP, VP], I),
    "hs_ba_drop_inactive_residuals": ([VP, VP], I),
    "hs_ba_remove_points": ([VP, I, VP], I),
    "hs_ba_remove_points_without_residuals": ([VP, VP, VP], I),
    "hs_ba_remove_frame": ([VP, I, I], I),
    "hs_ba_make_idx": ([VP, VP, VP, VP], I),
    "hs_ba_get_structure": ([VP] * 5, I),
    "hs_ba_get_marginal_prior": ([VP, VP, VP], I),
    "hs_ba_synchronize": ([VP], I),
    "hs_ba_get_point_state": ([VP] * 6, I),
    "hs_ba_get_last_residuals": ([VP, VP, VP], I),
    "hs_ba_set_last_residuals": ([VP, I, VP, VP, VP], I),
    "hs_ba_flag_points_for_removal": ([VP, I, VP, I, VP, VP, VP, VP], I),
    # test hook (not in the header): the per-point rule of hs_ba_flag_points_for_removal on the host
    "hs_debug_flag_rule": ([I, I, I, C.c_float, C.c_float, I, I, I], I),
    "hs_debug_state_size": ([], I),
    "hs_debug_get_state": ([VP, VP], I),
    "hs_debug_nullspace_error": ([VP, VP], I),
    "hs_debug_set_state": ([VP, VP], I),
    "hs_comm_get_unique_id": ([VP], I),
    "hs_comm_init": ([VP, VP, I, I], I),
    "hs_comm_size": ([VP, VP, VP], I),
    "hs_comm_set_timeout": ([VP, I], I),
    "hs_ba_set_event_timing": ([VP, I], I),
    "hs_ba_get_frame_eval": ([VP, VP, VP], I),
    # test hooks (not in the header): an in-process rank group on one device, the multi-rank exchange by copies
    "hs_ba_debug_group": ([VP, I, I], I),
    "hs_ba_group_linearize": ([VP, I, I, VP], I),
    "hs_ba_group_iterate": ([VP, I, I, I, VP], I),
    # test hooks (not in the header): a stale adjoint upload, a stalled stream
    "hs_debug_stale_adjoints": ([VP, I], I),
    "hs_debug_stall": ([VP, I], I),
    # include/hs_track.h
    "hs_tracker_create": ([VP, VP, I, I, I, I, VP], I),
    "hs_tracker_destroy": ([VP], None),
    "hs_tracker_set_ref": ([VP, VP, C.c_float, VP, I, VP, VP, VP, VP], I),
    "hs_tracker_get_ref": ([VP, I, VP, VP, VP, VP, VP], I),
    "hs_tracker_set_frame": ([VP, VP, C.c_float], I),
    "hs_tracker_calc_res": ([VP, I, VP, VP, C.c_float, VP, VP, VP, VP], I),
    "hs_tracker_track": ([VP, VP, VP, I, VP, VP, VP, VP], I),
    "hs_tracker_track_tries": ([VP, I, VP, VP, VP, C.c_float, VP, VP, VP, VP, VP, VP], I),
    "hs_tracker_get_lm_log": ([VP, I, I, VP, VP, VP, VP, VP], I),
    "hs_tracker_last_ms": ([VP, VP], I),
    "hs_tracker_set_event_timing": ([VP, I], I),
    "hs_tracker_last_stats": ([VP, I, VP, VP, VP], I),
    "hs_tracker_launch_info": ([VP, VP, VP], I),
    "hs_tracker_set_frame_raw": ([VP, VP, C.c_float], I),
    "hs_tracker_set_ref_ba": ([VP, VP, I, C.c_float, VP], I),
    "hs_tracker_frame_texels": ([VP, I, VP], I),
    "hs_tracker_frame_to_ba": ([VP, VP, I], I),
    # include/hs_pyr.h
    "hs_dir_pyramid": ([I, I, I, I, VP, VP, VP], I),
    # include/hs_trace.h
    "hs_tracer_create": ([VP, VP, I, I, I, I], I),
    "hs_tracer_destroy": ([VP], None),
    "hs_tracer_set_host_image": ([VP, I, VP], I),
    "hs_tracer_add_points": ([VP, I, VP, VP, VP], I),
    "hs_tracer_clear": ([VP], I),
    "hs_tracer_set_state": ([VP] * 6, I),
    "hs_tracer_set_types": ([VP, VP], I),
    "hs_tracer_activate": ([VP, VP, I, VP, VP, I, VP, VP, VP, VP, I, VP, I, VP, VP, VP, VP, VP, VP], I),
    "hs_tracer_get_distance_map": ([VP, VP], I),
    "hs_tracer_compact": ([VP, VP], I),
    "hs_tracer_activate_ba": ([VP, VP, I, VP, VP, VP, I, VP, I, VP, VP, VP, VP, VP], I),
    "hs_tracer_compact_device": ([VP, VP, VP, VP], I),
    "hs_tracer_get_act_inputs": ([VP] * 11, I),
    # test hooks (not in the header, no device work): the formed activation inputs and the mirror rule on the host
    "hs_debug_act_inputs": ([VP, I, VP, VP, VP, VP, VP, VP, VP], I),
    "hs_debug_act_mirror": ([I, I, VP, VP, VP, VP], I),
    "hs_debug_commit_count": ([VP], I),
    "hs_tracer_trace_ba": ([VP, VP, I, VP, VP, VP, C.c_float, VP], I),
    "hs_tracer_get_trace_inputs": ([VP, VP, VP], I),
    # test hook (not in the header, no device work): the formed trace inputs on the host
    "hs_debug_trace_hosts": ([VP, I, VP, VP, VP, VP, VP, VP, VP, C.c_float, VP], I),
    "hs_tracer_set_frame": ([VP, VP], I),
    "hs_tracer_set_frame_raw": ([VP, VP], I),
    "hs_tracer_trace": ([VP, I, VP, VP], I),
    "hs_tracer_get_points": ([VP] * 12, I),
    "hs_tracer_reinit": ([VP], I),
    "hs_tracer_last_stats": ([VP, VP, VP], I),
    # include/hs_select.h
    "hs_selector_create": ([VP, VP, I, I, I], I),
    "hs_selector_destroy": ([VP], None),
    "hs_selector_make_maps": ([VP, I, VP, VP, VP, VP, C.c_float, I, C.c_float, VP, VP], I),
    "hs_selector_make_maps_raw": ([VP, I, VP, C.c_float, I, C.c_float, VP, VP], I),
    "hs_selector_get_potential": ([VP, VP], I),
    "hs_selector_set_potential": ([VP, I], I),
    "hs_selector_last_stats": ([VP, VP, VP], I),
    # include/hs_refine.h
    "hs_refiner_create": ([VP, I, I, I, VP], I),
    "hs_refiner_destroy": ([VP], None),
    "hs_refiner_set_frames": ([VP, VP, VP, C.c_float, C.c_float], I),
    "hs_refiner_set_points": ([VP, I, VP, VP, VP, VP], I),
    "hs_refiner_refine": ([VP, VP, VP, VP, VP, VP], I),
    "hs_refiner_calc_res": ([VP, VP, VP, VP, VP, VP, VP, VP], I),
    "hs_refiner_get_points": ([VP, VP, VP, VP], I),
    "hs_refiner_get_log": ([VP, I, VP], I),
    "hs_refiner_last_ms": ([VP, VP], I),
    # include/hs_undist.h
    "hs_undist_make_remap": ([VP, VP, VP, VP], I),
    "hs_undist_make_photometric": ([VP, VP, I, VP, VP, VP], I),
    "hs_undistorter_create": ([VP, I, VP], I),
    "hs_undistorter_destroy": ([VP], None),
    "hs_undistorter_set_photometric": ([VP, VP, VP], I),
    "hs_undistorter_set_remap": ([VP, VP, VP], I),
    "hs_undistorter_get_K": ([VP, VP], I),
    "hs_undistorter_get_remap": ([VP, VP, VP], I),
    "hs_undistorter_apply": ([VP, VP, VP, VP], I),
    "hs_undistorter_time_kernel": ([VP, VP, I, I, VP], I),
    "hs_tracker_set_frame_u8": ([VP, VP, VP, C.c_float], I),
    "hs_tracer_set_frame_u8": ([VP, VP, VP], I),
    # include/hs_extract.h
    "hs_extractor_create": ([VP, I, I, I, I, VP], I),
    "hs_extractor_destroy": ([VP], None),
    "hs_extractor_extract": ([VP, VP, VP, VP], I),
    "hs_extractor_extract_selected": ([VP, VP, VP, VP], I),
    "hs_extractor_extract_u8": ([VP, VP, VP, VP, VP], I),
    "hs_extractor_get": ([VP] * 6, I),
    "hs_extractor_last_stats": ([VP, VP], I),
    "hs_fast_params_default": ([VP], None),
    "hs_extractor_extract_fast": ([VP, VP, VP, VP], I),
    "hs_extractor_extract_fast_u8": ([VP, VP, VP, VP, VP], I),
    "hs_extractor_extract_fast_image": ([VP, VP, VP, VP], I),
    "hs_extractor_get_fast": ([VP] * 6, I),
    # test hook (not in the header): one width of the last fast extract's Ssc search
    "hs_debug_fast_width": ([VP, I, VP, VP, VP, VP, I], I),
    "hs_tracer_add_keys": ([VP, VP, I, VP], I),
    # include/hs_flow.h
    "hs_flow_create": ([VP, I, I, I, I], I),
    "hs_flow_destroy": ([VP], None),
    "hs_flow_set_first": ([VP, VP, I, VP], I),
    "hs_flow_set_first_extracted": ([VP, VP, VP], I),
    "hs_flow_track": ([VP, VP, C.c_float, VP], I),
    "hs_flow_track_extracted": ([VP, VP, C.c_float, VP], I),
    "hs_flow_track_u8": ([VP, VP, VP, C.c_float, VP], I),
    "hs_flow_get": ([VP] * 8, I),
    "hs_flow_mean_flow": ([VP, VP], I),
    "hs_flow_mean_flow_device": ([VP, VP], I),
    "hs_flow_calc": ([VP, VP, VP, I, VP, VP, VP, VP, VP], I),
    "hs_flow_get_pyramid": ([VP, I, I, VP, VP, VP, VP], I),
    "hs_flow_last_stats": ([VP, VP, VP, VP], I),
    # include/hs_image.h
    "hs_image_create": ([VP, I, I, I, I], I),
    "hs_image_destroy": ([VP], None),
    "hs_image_set_u8": ([VP, VP, VP], I),
    "hs_image_set_raw": ([VP, VP], I),
    "hs_image_get": ([VP, I, VP, VP, VP], I),
    "hs_image_last_stats": ([VP, VP], I),
    "hs_tracker_set_frame_image": ([VP, VP, C.c_float], I),
    "hs_tracer_set_frame_image": ([VP, VP], I),
    "hs_tracer_set_host_image_from": ([VP, I, VP], I),
    "hs_selector_make_maps_image": ([VP, I, VP, C.c_float, I, C.c_float, VP, VP], I),
    "hs_extractor_extract_image": ([VP, VP, VP, VP], I),
    "hs_flow_track_image": ([VP, VP, C.c_float, VP], I),
    "hs_flow_set_first_image": ([VP, VP, I, VP], I),
    "hs_image_to_ba": ([VP, VP, I], I),
    # include/hs_init.h
    "hs_refiner_set_first_image": ([VP, VP, C.c_float], I),
    "hs_refiner_set_second_image": ([VP, VP, C.c_float], I),
    "hs_refiner_set_points_flow": ([VP, VP, VP, VP], I),
    "hs_refiner_get_videpth": ([VP, VP], I),
    "hs_refiner_seed_ba": ([VP, VP, I, VP, VP, VP], I),
    "hs_refiner_set_points_twoview": ([VP, VP, VP], I),
    # include/hs_twoview.h
    "hs_twoview_create": ([VP, I, I, VP], I),
    "hs_twoview_destroy": ([VP], None),
    "hs_twoview_fit": ([VP, I, VP, VP, VP, I, VP, VP], I),
    "hs_twoview_fit_flow": ([VP, VP, I, VP, VP], I),
    "hs_twoview_get": ([VP] * 8, I),
    "hs_twoview_last_result": ([VP, VP], I),
    "hs_twoview_get_rt": ([VP] * 8, I),
    "hs_twoview_last_stats": ([VP, VP], I),
    "hs_twoview_score_models": ([VP, I, VP, VP, I, VP], I),
    "hs_twoview_check_rt": ([VP, I, VP, VP, VP], I),
    "hs_twoview_rng_seed": ([VP, C.c_uint64], I),
    "hs_twoview_rng_skip": ([VP, C.c_uint64], I),
    "hs_twoview_rng_state": ([VP, VP], I),
    "hs_twoview_draw": ([VP, I, VP, I, VP, VP], I),
    "hs_twoview_fit_flow_drawn": ([VP, VP, I, VP], I),
    "hs_twoview_get_sets": ([VP, VP], I),
    "hs_twoview_last_draw_stats": ([VP, VP], I),
    # include/hs_map.h
    "hs_map_create": ([VP, I, I], I),
    "hs_map_destroy": ([VP], None),
    "hs_ba_attach_map": ([VP, VP], I),
    "hs_map_retire_points": ([VP, I, VP, VP], I),
    "hs_map_size": ([VP, VP, VP], I),
    "hs_map_frame_counts": ([VP, I, VP, VP], I),
    "hs_map_get_records": ([VP, I, I, VP], I),
    "hs_map_clear": ([VP], I),
    "hs_map_refresh_cloud": ([VP, VP, I, VP, VP, I, VP, VP], I),
    "hs_map_cloud_device": ([VP, VP, VP, VP], I),
    "hs_frame_marg_params_default": ([VP], I),
    "hs_ba_flag_frames_for_marginalization": ([VP] * 6, I),
    # test hook (not in the header): the frame rule of hs_ba_flag_frames_for_marginalization on the host
    "hs_debug_frame_rule": ([I] + [VP] * 8, I),
}

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C h-slam_amd/csrc` "
                           "(there is no CPU fallback for the hot path)")
    lib = C.CDLL(LIB_PATH)
    for name, (args, res) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


class HsError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise HsError(f"hs call failed ({rc}): {load().hs_last_error().decode(errors='replace')}")


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def default_params():
    p = hs_params()
    check(load().hs_params_default(C.byref(p)))
    return p
