/*
 * hs_image.h — one device-resident camera frame on MI355X, shared by every consumer of the image.
 *
 * Replaces what the reference's Frame constructor builds once per camera image (Src/Frame.cpp: DirPyr,
 * absSquaredGrad and cvImgL, read by the tracker, traceNewCoarse, PixelSelector, ExtractFeatures, the initializer's
 * flow and EnergyFunctional::insertFrame).  The raw u8 frame is uploaded once, undistorted once and its pyramid built
 * once, in two kernels (hs_k_img_levels, hs_k_img_grads); each consumer then copies what it reads, device to device,
 * into its own buffers.  No image-sized buffer crosses the host after the upload.
 *
 * Same conventions as hs_extract.h: plain C, status codes from hs_types.h with the message in hs_last_error(), the
 * image owns its device memory, its staging of the raw frame and its own HIP stream, host buffers are the caller's
 * and copied in / out, one image per calling thread.
 *
 * The contract is bit-identity with the existing chain: level l, every texel lane, absSquaredGrad[l] and cvImgL are
 * what hs_undistorter_apply (include/hs_undist.h, the kernel's arithmetic) followed by hs_dir_pyramid
 * (include/hs_pyr.h) produce.
 *
 * Ordering.  hs_image_set_* returns without waiting for the device.  A consumer's entry makes its own stream wait for
 * the image's last set, copies on its own stream and leaves an event behind; the image's next set waits for every
 * such event before it overwrites a level.  None of it blocks the host, so a frame's hand-off to all consumers and
 * the next frame's upload are enqueued back to back.  The caller's `raw` / `fimg` is copied to pinned staging before
 * a set returns and may be reused at once.  The undistorter's tables are read where they lie: replace them
 * (hs_undistorter_set_photometric, _set_remap) only after the sets that used them completed (hs_image_get waits).
 * The consumers' entries return as soon as their work is enqueued, unless the entry they mirror waits for a result
 * (the selector's counts, the extractor's key count, the flow's counters).  hs_tracker_frame_texels names memory
 * that hs_tracker_set_frame_image fills on the tracker's stream without a host wait: hand that frame to the BA with
 * hs_image_to_ba, not with hs_ba_set_frame_image_device.
 */
#ifndef HS_IMAGE_H
#define HS_IMAGE_H

#include "hs_types.h"
#include "hs_ba.h"
#include "hs_extract.h"
#include "hs_flow.h"
#include "hs_select.h"
#include "hs_trace.h"
#include "hs_track.h"
#include "hs_undist.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hs_image hs_image;

/* width / height: CalibData::Width / Height, each >= 1; n_levels: DirPyrLevels, the range hs_tracker_create accepts
   (1 <= n_levels <= HS_TRK_MAXLEV), with a top level of at least 1 x 1.  A violation is HS_ERR_INVALID before any
   device call.  (Each consumer's own size rule is checked where the consumer is created.) */
int hs_image_create(hs_image** out, int device_id, int width, int height, int n_levels);
void hs_image_destroy(hs_image* im);

/* The frame as the camera's raw u8 frame (w_in*h_in bytes): uploaded into the image's own staging, undistorted and
   its pyramid built on the image's stream.  The undistorter must be on the image's device and its output size the
   image's size (HS_ERR_INVALID).  Returns without waiting for the device. */
int hs_image_set_u8(hs_image* im, hs_undistorter* u, const uint8_t* raw);
/* The frame as ImageData::fImgL (W*H floats).  No cvImgL is made: hs_image_get's img8_out,
   hs_extractor_extract_image and hs_flow_track_image return HS_ERR_STATE until the next hs_image_set_u8. */
int hs_image_set_raw(hs_image* im, const float* fimg);
/* Parity read-back of level lvl, all outputs nullable: dirpyr_out = w_l*h_l (I, dI/dx, dI/dy) triplets, absg_out =
   w_l*h_l floats (absSquaredGrad[lvl]), img8_out = W*H bytes (cvImgL; lvl must be 0).  HS_ERR_STATE before the
   first set.  Waits for the device. */
int hs_image_get(hs_image* im, int lvl, float* dirpyr_out, float* absg_out, uint8_t* img8_out);
/* Device time (ms) of the last set, from its first kernel to its last (HIP events on the image's stream); waits for
   that set. */
int hs_image_last_stats(hs_image* im, double* ms);

/* The consumers.  Every entry first checks, before any device call: the image is on the consumer's device and of
   its size and has the levels the consumer reads (HS_ERR_INVALID), and it holds a frame -- with a cvImgL where the
   consumer reads one (HS_ERR_STATE).  A failed entry changes nothing in the consumer. */

/* hs_tracker_set_frame_u8 / _raw: all of the tracker's levels (the image needs at least as many). */
int hs_tracker_set_frame_image(hs_tracker* t, hs_image* im, float ab_exposure);
/* hs_tracer_set_frame_u8 / _raw: level 0 as the frame to trace on. */
int hs_tracer_set_frame_image(hs_tracer* t, hs_image* im);
/* hs_tracer_set_host_image: level 0 as host slot `slot`'s image (allocated on first use). */
int hs_tracer_set_host_image_from(hs_tracer* t, int slot, hs_image* im);
/* hs_selector_make_maps_raw: level 0's texels and absSquaredGrad[0..2]; the image needs >= 3 levels. */
int hs_selector_make_maps_image(hs_selector* s, int frame_id, hs_image* im, float density, int recursions_left,
                                float th_factor, float* map_out, int* n_selected);
/* hs_extractor_extract_u8: cvImgL. */
int hs_extractor_extract_image(hs_extractor* e, hs_selector* s, hs_image* im, int* n_keys);
/* hs_flow_track_u8: cvImgL. */
int hs_flow_track_image(hs_flow* f, hs_image* im, float max_l1_error, int* n_good);
/* hs_flow_set_first with TransitImage = cvImgL copied device to device; the keys xy[n][2] are the host's (a caller that
   has its mvKeys from elsewhere than an extractor). */
int hs_flow_set_first_image(hs_flow* f, hs_image* im, int n, const float* xy);
/* hs_tracker_frame_to_ba without a tracker: level 0 becomes window frame `frame`'s image, the packed-texel refresh
   included, ordered on the device both ways. */
int hs_image_to_ba(hs_image* im, hs_ctx* ba, int frame);

#ifdef __cplusplus
}
#endif
#endif /* HS_IMAGE_H */
