/*
 * hs_undist.h — raw 8-bit camera frames undistorted on MI355X.
 *
 * Replaces DatasetReader::undistort (Include/DatasetLoader.h:436-506): the photometric correction per pixel
 * (Src/PhotometricDistorter/photometricUndistorter.cpp:121-146) and the full-image cv::remap through the table
 * GeometricUndistorter builds once per calibration (Src/GeometricUndistorter.cpp:161-194, 458-475), fused into one
 * kernel that reads the camera's u8 frame and writes ImageData::fImgL (and, optionally, cvImgL).  The contexts take
 * the raw frame directly (hs_tracker_set_frame_u8, hs_tracer_set_frame_u8): fImgL never exists on the host.
 *
 * Same conventions as hs_ba.h: plain C, caller-owned host buffers copied in / out, status codes from hs_types.h
 * with the message in hs_last_error(), no exception crosses the ABI, one undistorter per calling thread.
 *
 * The two table builders are host-only and need no device.  Not built: the stereo "rectify" branch
 * (cv::initUndistortRectifyMap; such callers bring their maps to hs_undistorter_set_remap) and OnlineCalib.
 *
 * The kernel's contract (cv::remap INTER_LINEAR, CV_32F maps, float source, constant 0 border, as arithmetic):
 *   sx = cvRound(remap_x * 32.f) (half to even), ix = sx >> 5, fx = (sx & 31) * (1.f / 32); the same for y;
 *   w0 = (1-fy)*(1-fx), w1 = (1-fy)*fx, w2 = fy*(1-fx), w3 = fy*fx in float;
 *   S(p at index i) = Binv[p] * vignette_inv[i] | Binv[p] | (float)p * vignette_inv[i] | (float)p
 *   (gamma and vignette | gamma | vignette | neither); a tap outside the input is 0;
 *   fImg = S00*w0 + S01*w1 + S10*w2 + S11*w3, summed left to right, unfused;  passthrough: fImg = S(p);
 *   img8 = sat8(B[sat8(fImg)]) with photometric tables, sat8(fImg) without (sat8: half to even, clamped 0..255).
 *   Non-finite values (a zero in the vignette) are unspecified.
 */
#ifndef HS_UNDIST_H
#define HS_UNDIST_H

#include "hs_types.h"
#include "hs_trace.h"
#include "hs_track.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Calibration.model */
enum { HS_CAM_PINHOLE = 0, HS_CAM_ATAN = 1, HS_CAM_RADTAN = 2, HS_CAM_EQUIDISTANT = 3, HS_CAM_KANNALABRANDT = 4 };
/* Calib.process */
enum { HS_UNDIST_CROP = 0, HS_UNDIST_NONE = 1, HS_UNDIST_USEK = 2 };

/* The monocular fields of a geometric calibration file (the yaml files of Extras/Calib), as the reference reads them. */
typedef struct hs_undist_calib {
  int model;            /* HS_CAM_* */
  int w_in, h_in;       /* Input.width / height */
  int w_out, h_out;     /* Output.width / height */
  int process;          /* HS_UNDIST_* */
  double K_in[4];       /* CameraL.K: fx fy cx cy; relative to the input size when cx < 1 && cy < 1 */
  double dist[4];       /* CameraL.distM (RadTan, EquiDistant, KannalaBrandt); dist[0] = CameraL.dist (Atan, Pinhole) */
  double desired_K[4];  /* Calib.desiK: fx fy cx cy relative to the output size (useK only) */
} hs_undist_calib;

/* GeometricUndistorter::LoadGeometricCalibration's monocular path: K_out = the K that goes with the undistorted
   images (makeOptimalK_crop | desired_K | K_in); remap_x / remap_y (w_out*h_out floats each) = the source
   coordinate of every output pixel, (-1, -1) where the reference's validity pass rejects it.  HS_UNDIST_NONE
   requires equal sizes; its images pass through (the table is still filled, as the reference fills it). */
int hs_undist_make_remap(const hs_undist_calib* calib, float K_out[4], float* remap_x, float* remap_y);

/* PhotometricUndistorter's tables.  G256 (nullable => identity): the camera response, exactly 256 strictly
   increasing entries (a C pointer carries no length: callers that know one check it, as hslam_amd.undistort does),
   normalised to 0..255 into Binv; B = its inverse by UpdateGamma's loop (entries the loop does not assign are 0).
   vignette (nullable => vignette_inv untouched): n_in u16 values, vignette_inv[i] = max / v[i]. */
int hs_undist_make_photometric(const float* G256, const uint16_t* vignette, int n_in, float Binv[256], float B[256],
                               float* vignette_inv);

typedef struct hs_undistorter hs_undistorter;

/* Builds the table of `calib` and places it on device `device_id`; no photometric tables. */
int hs_undistorter_create(hs_undistorter** out, int device_id, const hs_undist_calib* calib);
void hs_undistorter_destroy(hs_undistorter* u);
/* Replaces the photometric tables: G256 (256 floats) and vignette (w_in*h_in u16), either nullable (both null:
   no photometric correction).  Complete on the device at return. */
int hs_undistorter_set_photometric(hs_undistorter* u, const float* G256, const uint16_t* vignette);
/* Replaces the built table with the caller's own maps (w_out*h_out floats each, finite, within +-32767); a
   passthrough calibration stops passing through.  Complete on the device at return. */
int hs_undistorter_set_remap(hs_undistorter* u, const float* remap_x, const float* remap_y);
int hs_undistorter_get_K(const hs_undistorter* u, float K_out[4]);
/* the table in use, in its float form (nullable outputs) */
int hs_undistorter_get_remap(const hs_undistorter* u, float* remap_x, float* remap_y);
/* Standalone: uploads raw (w_in*h_in bytes), undistorts on the device and copies back fimg_out (nullable,
   w_out*h_out floats: fImgL) and img8_out (nullable, w_out*h_out bytes: cvImgL). */
int hs_undistorter_apply(hs_undistorter* u, const uint8_t* raw, float* fimg_out, uint8_t* img8_out);

/* Measurement (tools/undist_time.py): uploads raw once, then `warmup` untimed and `launches` timed back-to-back
   launches of the kernel (fImg only) between one pair of device events; *ms_per_launch = elapsed / launches. */
int hs_undistorter_time_kernel(hs_undistorter* u, const uint8_t* raw, int warmup, int launches, float* ms_per_launch);

/* The frame to track / to trace on as the camera's raw u8 frame: w_in*h_in bytes are uploaded on the consumer's own
   stream, and the consumer's pyramid is built from them, each level-0 pixel undistorted as it is written (the result
   is that of hs_undistorter_apply followed by hs_tracker_set_frame_raw / hs_tracer_set_frame_raw).  The undistorter
   must be on the consumer's device and its output size the consumer's size, else HS_ERR_INVALID. */
int hs_tracker_set_frame_u8(hs_tracker* t, hs_undistorter* u, const uint8_t* raw, float ab_exposure);
int hs_tracer_set_frame_u8(hs_tracer* t, hs_undistorter* u, const uint8_t* raw);

#ifdef __cplusplus
}
#endif
#endif /* HS_UNDIST_H */
