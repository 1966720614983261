/*
 * hs_flow.h — the initializer's keypoint tracking on MI355X: pyramidal Lucas-Kanade flow of the first frame's keys.
 *
 * Replaces Initializer::FindMatches (Src/Initializer.cpp:341-399): cv::calcOpticalFlowPyrLK with a 15x15 window,
 * maxLevel 2, criteria COUNT+EPS (30, 0.01), minEigThreshold 1e-4, on every keypoint of the first frame, run on every
 * frame until initialization succeeds; its bookkeeping (MatchedPtsBkp, MatchedPts, MatchedStatus, TransitImage); and
 * Initializer::ComputeMeanOpticalFlow (:1313-1328).  The first frame's keys and both images are read where
 * hs_extractor_extract left them on the device (mvKeys, cvImgL): no image-sized buffer crosses the host.
 *
 * Same conventions as hs_extract.h: plain C, status codes from hs_types.h with the message in hs_last_error(), the
 * context owns its device memory and its own HIP stream, host buffers are the caller's and copied in / out, one
 * context per calling thread.  A call is complete on the device when it returns.
 *
 * Not built: MatchIndirect.  The H/F RANSAC and the triangulation of Initializer::Initialize are include/hs_twoview.h.
 *
 * Parity.  OpenCV is not a dependency of this project, so the contract below restates the scalar path of OpenCV 4's
 * calcOpticalFlowPyrLK for 8-bit single-channel input as arithmetic; tests/flow_ref.py states the same arithmetic in
 * numpy and is what the kernels are compared with, bit for bit.  Parity with an OpenCV binary is not pinned.  One
 * deliberate deviation: the sums over the window are exact integer sums converted to float once, where OpenCV
 * accumulates in float in a lane order that depends on its build.
 *
 * The contract, as arithmetic.  WIN = 15, half = 7.0f, r(i, n) = -i if i < 0, 2n-2-i if i >= n, else i.
 *   Pyramid.  Level 0 is the W x H u8 image.  Level l+1 exists iff l < 2 and both ((w_l+1)/2, (h_l+1)/2) are > 15
 *           (64x48 has 2 levels, 30x30 has 1).  pyrDown, all integer, k = 1 4 6 4 1:
 *           hor[y][x] = sum_j k[j] * src[y][r(2x+j-2, w)];  out[y][x] = (sum_j k[j] * hor[r(2y+j-2, h)][x] + 128) >> 8;
 *           the output is ((w+1)/2) x ((h+1)/2).
 *   Derivative (Scharr, int16, of the previous image's levels).  t0 = 3*(I[r(y-1)] + I[r(y+1)]) + 10*I[y],
 *           t1 = I[r(y+1)] - I[r(y-1)];  dx = t0[r(x+1)] - t0[r(x-1)];  dy = 3*(t1[r(x+1)] + t1[r(x-1)]) + 10*t1[x].
 *           Both lie within +-4080.
 *   Reads outside a level.  Image taps use r() on both axes; derivative taps are 0.  No tap lies more than 15 px
 *           outside, by the bounds tests below.
 *   Per point: status = 1, err = 0.  For l = L .. 0 (L the top level that exists):
 *     s = 2^-l, p = prev_xy * s.  Top level: g = init_xy * s if a guess is given, else g = p; below: g = 2 * (the
 *           output so far).  The output so far = g.
 *     Previous window.  p -= half.  Test px >= -15 && px < w_l && py >= -15 && py < h_l on the floats (NaN and huge
 *           values fail it); only then convert to int.  Failure: status = 0 if l == 0; next level.
 *     Weights.  ip = floor(p), a = px - ipx, b = py - ipy;  iw00 = rint((1-a)*(1-b)*16384), iw01 = rint(a*(1-b)*16384),
 *           iw10 = rint((1-a)*b*16384), each product rounded in float, left to right, rint half to even;
 *           iw11 = 16384 - iw00 - iw01 - iw10.
 *     Patch.  For the 15 x 15 window pixels (x, y), taps at ip + (x, y), +(1, 0), +(0, 1), +(1, 1) with weights iw00,
 *           iw01, iw10, iw11:  I = (sum taps*iw + 256) >> 9;  Ix, Iy = (sum derivative taps*iw + 8192) >> 14.
 *     Normal matrix.  A11 = (float)sum Ix^2 * 2^-20, A12 = (float)sum Ix*Iy * 2^-20, A22 = (float)sum Iy^2 * 2^-20,
 *           each sum an exact integer converted to float once.  D = A11*A22 - A12*A12;
 *           minEig = (A22 + A11 - sqrt((A11-A22)*(A11-A22) + 4*A12*A12)) / 450, all float, every operation rounded
 *           and none fused, sqrt and the division correctly rounded.  (double)minEig < 1e-4 or D < FLT_EPSILON:
 *           status = 0 if l == 0; next level (the output so far stays g).  D = 1 / D.
 *     Iterations.  q = g - half, prevDelta = 0.  For j = 0 .. 29:  the bounds test on q (failure: status = 0 if
 *           l == 0; leave);  weights from q;  diff = ((sum next taps*iw + 256) >> 9) - I;
 *           b1 = (float)sum diff*Ix * 2^-20, b2 = (float)sum diff*Iy * 2^-20 (exact integer sums);
 *           delta = ((A12*b2 - A22*b1)*D, (A12*b1 - A11*b2)*D);  q += delta;  the output so far = q + half;
 *           (double)dx^2 + (double)dy^2 <= 0.01*0.01 (doubles): leave;
 *           j > 0 and |dx + prevDelta.x| < 0.01 and |dy + prevDelta.y| < 0.01 (float sums against the double 0.01):
 *           the output so far -= 0.5 * delta; leave;  prevDelta = delta.
 *     Error.  l == 0 and status still 1:  e = output - half;  the bounds test (failure: status = 0);  weights from e;
 *           err = (float)sum |((sum next taps*iw + 256) >> 9) - I| * (1.f / 7200).  Where status is 0, err is 0.
 *   FindMatches.  good[i] = status[i] && err[i] < max_l1_error.  The previous points of a call (MatchedPtsBkp) are
 *           the outputs of the call before it, those of failed points included (on the first call: the first frame's
 *           points), the guess equals the previous points, and the previous image is the image of the call before.
 */
#ifndef HS_FLOW_H
#define HS_FLOW_H

#include "hs_types.h"
#include "hs_extract.h"
#include "hs_undist.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hs_flow hs_flow;

/* width, height >= 16 (a 15 px reflected border needs 16 px to reflect); capacity >= 1: the most points of one call.
   A violation is HS_ERR_INVALID before any device call. */
int hs_flow_create(hs_flow** out, int device_id, int width, int height, int capacity);
void hs_flow_destroy(hs_flow* f);

/* Initialize()'s first-frame branch: TransitImage = img8 (W*H bytes, host), FirstFramePts = mvbPrevMatched =
   xy[n][2] (host; nullable when n == 0).  n > capacity: HS_ERR_INVALID, the state unchanged. */
int hs_flow_set_first(hs_flow* f, const uint8_t* img8, int n, const float* xy);
/* The same from the extractor's last extract: cvImgL and the keys, device to device; *n (nullable) = the keys taken.
   The extractor must be on the flow's device and of its size and hold no more keys than `capacity`
   (HS_ERR_INVALID), and must have extracted (HS_ERR_STATE).  The image is that of its last extract call. */
int hs_flow_set_first_extracted(hs_flow* f, hs_extractor* e, int* n);

/* One FindMatches against the new frame's cvImgL (host); *n_good (nullable) = its return value.  Before a first
   frame: HS_ERR_STATE. */
int hs_flow_track(hs_flow* f, const uint8_t* img8, float max_l1_error, int* n_good);
/* The same with the new frame's cvImgL read where the extractor's last extract left it. */
int hs_flow_track_extracted(hs_flow* f, hs_extractor* e, float max_l1_error, int* n_good);
/* The same with cvImgL made from the camera's raw frame (w_in*h_in bytes, host) on the flow's stream; the
   undistorter's output size must be the flow's size. */
int hs_flow_track_u8(hs_flow* f, hs_undistorter* u, const uint8_t* raw, float max_l1_error, int* n_good);

/* The tracked state, all nullable: *n, first_xy[n][2] (FirstFramePts), prev_xy[n][2] (MatchedPtsBkp), xy[n][2]
   (MatchedPts), status[n], err[n] of the last track, good[n] (MatchedStatus).  Before the first track prev_xy and xy
   are the first frame's points and status, err and good are 0. */
int hs_flow_get(hs_flow* f, int* n, float* first_xy, float* prev_xy, float* xy, uint8_t* status, float* err,
                uint8_t* good);
/* ComputeMeanOpticalFlow(MatchedPtsBkp, MatchedPts) over the good points, on the host, with the reference's
   accumulate into an int: acc = (int)(acc + norm), norm = (float)sqrt((double)dx^2 + (double)dy^2), the result
   (float)acc / (float)count (NaN when no point is good).  Before a track: HS_ERR_STATE. */
int hs_flow_mean_flow(hs_flow* f, float* mean);
/* The same value, bit for bit, made on the device: every norm in parallel, then the truncating accumulation as one
   ordered chain in key order (it is not associative: the float sum rounds before the truncation).  The read-back is
   the 4 bytes of the result. */
int hs_flow_mean_flow_device(hs_flow* f, float* mean);

/* One stand-alone calcOpticalFlowPyrLK between two given images (host) for n <= capacity points; init_xy nullable
   (no guess: the flow starts at prev_xy); xy_out[n][2], status_out[n], err_out[n] nullable.  Does not touch the
   tracked state. */
int hs_flow_calc(hs_flow* f, const uint8_t* prev8, const uint8_t* next8, int n, const float* prev_xy,
                 const float* init_xy, float* xy_out, uint8_t* status_out, float* err_out);

/* A level of the last calc's or track's pyramids: which = 0 the previous image, 1 the next; img_out[w*h] and
   deriv_out[w*h][2] (int16 dx, dy; also kept for a next image, which a track makes the next call's previous one)
   nullable; *w, *h (nullable) the level's size.  A level that does not exist: HS_ERR_INVALID; before any calc or
   track: HS_ERR_STATE. */
int hs_flow_get_pyramid(hs_flow* f, int which, int level, uint8_t* img_out, int16_t* deriv_out, int* w, int* h);
/* last calc / track: device time (ms, HIP events on the flow's stream) from the first kernel to the last, the sum of
   the Lucas-Kanade iterations run over all points and levels, and the levels used.  All nullable. */
int hs_flow_last_stats(hs_flow* f, double* ms, long long* iterations, int* levels);

#ifdef __cplusplus
}
#endif
#endif /* HS_FLOW_H */
