/*
 * hs_init.h — the initializer's hand-off on MI355X: from "second frame tracked" to the first window's points, with
 * the frames, the keys and the new points staying on the device.
 *
 * Replaces, around DirectRefinement (include/hs_refine.h):
 *   hs_refiner_set_first_image / _set_second_image   FirstFrame / SecondFrame ->frame->DirPyr[0] taken from a device
 *                                                    image (include/hs_image.h) instead of two host W*H*3 arrays
 *   hs_refiner_set_points_flow                       the ctor's Pnt set-up (Src/Initializer.cpp:1362-1382) with
 *                                                    mvKeys read where the flow context holds them (FirstFramePts)
 *   hs_refiner_set_points_twoview                    the same with vbTriangulated and mvIniP3D[i].z read where the two-view
 *                                                    fit (include/hs_twoview.h) left them
 *   hs_refiner_get_videpth                           Initializer::videpth (Src/Initializer.cpp:155-159) after
 *                                                    DirectRefinement's write-back (:1393-1397)
 *   hs_refiner_seed_ba                               System::InitFromInitializer's point loop (Src/System.cpp:265-290)
 *
 * Same conventions as hs_image.h: plain C, status codes from hs_types.h with the message in hs_last_error(), host
 * buffers are the caller's and copied in / out, every entry checks device, size and state before any device call, and a
 * failed entry changes nothing unless its comment says otherwise.
 *
 * Initializer::FindTransformation (the H / F RANSAC and the triangulation) is include/hs_twoview.h: its vbTriangulated
 * and mvIniP3D[i].z / MedianDepth reach the refiner device to device through hs_refiner_set_points_twoview, and its pose
 * (R, t / MedianDepth of the result record) is hs_refiner_refine's start.  What stays with the caller is the cv::RNG draw
 * of mvSets and the nmatches test of Src/Initializer.cpp:129-137, which reads the record's n_triangulated.  A caller with
 * a fit of its own still hands `triangulated` and `z` to hs_refiner_set_points_flow.
 * The frames of the first window stay with the existing calls: frame 0 is hs_ba_insert_frame + hs_image_to_ba, the
 * second frame's pose is the refined Pose through hs_ba_insert_frame + hs_ba_add_residuals_to_newest.
 *
 * Parity status.  Frames: the refiner's texels are the image's level 0, so calcResAndGS, Refine's log, the pose and
 * every point plane are bit-identical to hs_image_get + hs_refiner_set_frames.  Points: every plane is bit-identical
 * to hs_refiner_set_points on the same keys.  Seeding: the window (point state, structure, lastResiduals) and what
 * linearize / optimize make of it are bit-identical to the host loop (videpth read-back, hs_tracer_add_points at
 * +0.5, hs_ba_insert_points with has_depth_prior, hs_ba_set_last_residuals (none, IN)).  Two deviations from the
 * reference, both on keys the reference handles by reading outside its image or not at all: `why` code 3 below, and
 * keys outside the image are refused (hs_refiner_set_points' rule).
 */
#ifndef HS_INIT_H
#define HS_INIT_H

#include "hs_types.h"
#include "hs_ba.h"
#include "hs_flow.h"
#include "hs_image.h"
#include "hs_refine.h"
#include "hs_twoview.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Level 0 of `im` becomes the refiner's first / second frame: copied device to device on the refiner's stream behind
   the image's last set; returns without waiting, and the image may be set again at once (hs_image.h, Ordering).  The
   image must be on the refiner's device and of its size (HS_ERR_INVALID) and hold a frame (HS_ERR_STATE).
   ab_exposure: FrameShell::ab_exposure, as hs_refiner_set_frames takes it.  The two frames are set independently (the
   initializer takes its first frame once; every later frame is a candidate second frame); hs_refiner_refine and
   hs_refiner_calc_res need both, from these entries or from hs_refiner_set_frames, which sets both. */
int hs_refiner_set_first_image(hs_refiner* r, hs_image* im, float ab_exposure);
int hs_refiner_set_second_image(hs_refiner* r, hs_image* im, float ab_exposure);

/* hs_refiner_set_points with (u, v) = the flow's FirstFramePts (hs_flow_set_first / _set_first_extracted; never
   MatchedPts, which moves with every track), read on the device.  triangulated[n], z[n]: the two-view fit's
   vbTriangulated and mvIniP3D[i].z from the host, n = the flow's first-frame count.  The flow must be on the refiner's
   device and of its size and hold at least one point (HS_ERR_INVALID), after a first frame (HS_ERR_STATE).
   hs_refiner_set_points' key range rule (finite, 0 <= u <= W - 1, 0 <= v <= H - 1) is checked on the device: on a
   violation the call returns HS_ERR_INVALID and the refiner holds no points.  Waits for the device (one 4-byte
   read-back: the violation count). */
int hs_refiner_set_points_flow(hs_refiner* r, hs_flow* f, const uint8_t* triangulated, const float* z);

/* hs_refiner_set_points_flow with `triangulated` and `z` taken device to device from the last fit of `tv`: z[i] =
   mvIniP3D[i].z / median_depth (Src/Initializer.cpp:146-148).  The flow's rules are hs_refiner_set_points_flow's.
   HS_ERR_STATE, nothing changed: the last fit of `tv` did not succeed (result.ok == 0, a refused call, or a debug entry
   since), or it was not hs_twoview_fit_flow on this flow's current first frame and key count.  Another device:
   HS_ERR_INVALID. */
int hs_refiner_set_points_twoview(hs_refiner* r, hs_flow* f, hs_twoview* tv);

/* Parity read-back, videpth[n]: -1 where the key is not triangulated; else the refined idepth where the point is
   good, 1 / z where it is not.  Before a refine this is the constructor's array (1 / z or -1).  Legal once points are
   set (HS_ERR_STATE before). */
int hs_refiner_get_videpth(hs_refiner* r, float* videpth);

/* InitFromInitializer's point loop over the refiner's points, in mvKeys order, into window frame `frame` of `ba`.
   Legal once points and the first frame are set; before a refine the state is the constructor's.
     why_out[n] (nullable), per key: 0 seeded; 1 videpth <= 0; 2 energyTH not finite (one of the 8 colours of the
       ImmaturePoint constructor at (u + 0.5f, v + 0.5f) on the first frame is not finite); 3 (u + 0.5f, v + 0.5f)
       breaks hs_tracer_add_points' border rule (>= 2, < W - 3, < H - 3).  Code 3 is a deviation: the reference
       builds the point and reads outside its image there.  It is tested before the colours are read.
     A seeded key becomes one point of `frame`, in key order behind the frame's earlier points: (u + 0.5f, v + 0.5f),
       idepth = idepth_zero = videpth, hasDepthPrior (priorF as hs_ba_insert_points sets it), maxRelBaseline 0,
       numGoodResiduals 0, the constructor's colours and weights, no residual.  handles_out[n_seeded] (nullable, room
       for n) receives the points' handles, *n_seeded (nullable) their number.
     lastResiduals: the reference's pairs are value-initialised here, so a seeded point reads back through
       hs_ba_get_last_residuals as target (-1, -1), state (HS_RES_IN, HS_RES_IN) -- not activation's (none, OOB).
   The points are staged on the device; the caller's next commit (hs_ba_make_idx, or any call that commits) gathers
   them, ordered behind this call on the device.  The only read-backs are `why` (n bytes) and the count.
   Errors leave the refiner and the window unchanged: a multi-rank context, no points or no first frame
   (HS_ERR_STATE); another device, another image size, `frame` not a window frame (HS_ERR_INVALID); window points +
   seeded > the reserved capacity (HS_ERR_NOMEM, nothing staged). */
int hs_refiner_seed_ba(hs_refiner* r, hs_ctx* ba, int frame, uint8_t* why_out, int* handles_out, int* n_seeded);

#ifdef __cplusplus
}
#endif
#endif /* HS_INIT_H */
