/*
 * hs_extract.h — keyframe feature extraction on MI355X: the step between the selection map and the immature points.
 *
 * Replaces Frame::Extract -> FeatureDetector::ExtractFeatures (Src/Detector.cpp:31-131) with the shipped settings
 * (UseFAST = false, DoSubPix = false, Src/Settings.cpp:20-21): the raster scan of selectionMap's interior into
 * mvKeys (:59-66), the 7x7 Gaussian blur of cvImgL (:71), IC_Angle (:133-159) and the rotated-BRIEF descriptor
 * (computeOrbDescriptor, :91-131) of every key; and, with hs_tracer_add_keys, the loop of System::makeNewTraces
 * (Src/Mapping.cpp:225-247) that builds one ImmaturePoint per key.  The map is read where hs_selector_make_maps left
 * it and the keys go to the tracer device to device: no image-sized buffer crosses the host.
 *
 * Same conventions as hs_select.h: plain C, status codes from hs_types.h with the message in hs_last_error(), the
 * extractor owns its device memory and its own HIP stream, host buffers are the caller's and copied in / out, one
 * extractor per calling thread.  An extract is complete on the device when it returns; its result stays readable
 * (hs_extractor_get, hs_tracer_add_keys) until the next successful extract.
 *
 * The 256-pair sampling pattern (FeatureDetector::pattern) is an argument: H-SLAM passes its own table.
 *
 * The UseFAST = true branch (cv::FAST at minThFAST with non-maximum suppression, the sort by response and Ssc,
 * Src/Detector.cpp:47-55, :451-553) is hs_extractor_extract_fast: it fills the same result set, so every consumer of
 * the keys reads them as it reads the map branch's.  Its contract is the second block below.
 *
 * Not built: DoSubPix (cv::cornerSubPix), Frame::mGrid, CreateIndPyrs and
 * descriptor matching.  The live consumer of the keys and of cvImgL during initialization, Initializer::FindMatches'
 * Lucas-Kanade tracking, is hs_flow.h, which reads both where an extract left them.
 *
 * The contract, as arithmetic (W x H image, row-major):
 *   Keys.   for y in [19, H-19), then x in [19, W-19): key (x, y) where map[y*W + x] != 0; keys keep that order.
 *   Blur    (cv::GaussianBlur 7x7, sigma 2, BORDER_REFLECT_101 on u8, as 8-bit fixed point): weights w[0..6] = the
 *           normalised Gaussian exp(-(k-3)^2 / 8) in double, scaled by 256, rounded from the outer tap inward with
 *           the rounding error carried into the next tap, mirrored, centre = 256 - sum of the others:
 *           18 34 48 56 48 34 18.  r(i, n) = -i if i < 0, 2n-2-i if i >= n, else i.
 *           h[y][x] = sum_k w[k] * src[y][r(x+k-3, W)] (fits u16); v = sum_k w[k] * h[r(y+k-3, H)][x] (u32);
 *           blurred = (v + 32768) >> 16.  All integer.
 *   Angle   (IC_Angle on the unblurred image): umax[0..15] by InitUmax's rule for half patch 15;
 *           m10 = sum u*I(x+u, y+v), m01 = sum v*I(x+u, y+v) over |v| <= 15, |u| <= umax[|v|], in int32 (|m| < 2^24);
 *           angle = fastAtan2((float)m01, (float)m10), OpenCV's scalar form in float, every operation rounded and
 *           none fused: ax = |x|, ay = |y|, eps = (float)DBL_EPSILON;
 *           ax >= ay: c = ay / (ax + eps), c2 = c*c, a = (((p7*c2 + p5)*c2 + p3)*c2 + p1)*c;
 *           else:     c = ax / (ay + eps), a = 90 - the same polynomial in c;
 *           x < 0: a = 180 - a;  y < 0: a = 360 - a;
 *           p1, p3, p5, p7 = 0.9997878412794807f, -0.3258083974640975f, 0.1555786518463281f, -0.04432655554792128f,
 *           each multiplied in float by (float)(180 / pi).  Degrees in [0, 360].
 *   Descriptor.  rad = angle * (float)(pi / 180); a = (float)cos((double)rad), b = (float)sin((double)rad);
 *           bit i has taps p = pattern[2i], q = pattern[2i+1] (pattern[4i .. 4i+3] = p.x, p.y, q.x, q.y);
 *           val(p) = blurred[(y + rint(p.x*b + p.y*a)) * W + x + rint(p.x*a - p.y*b)], each product and each sum
 *           rounded in float, rint half to even; bit = val(p) < val(q), stored at desc[i / 8] bit i % 8.
 *   Bounds. Pattern entries lie within +-13 (checked at creation), so a rotated tap reaches at most 18 px; the angle's
 *           disc reaches 15 px; keys lie >= 19 px from every edge.  Every gather is in bounds by these rules.
 *
 * The FAST branch, as arithmetic (cvImgL I, u8, W x H; threshold t, num_features, tolerance, min_dist).  Where the
 * reference is undefined or leaves an order open, the rule here is the contract (DESIGN.md lists these deviations).
 * OpenCV is no dependency and parity with cv::FAST is not pinned: this text is.
 *   Corners (cv::FAST 9-16).  Ring offsets (dx, dy), k = 0..15: (0,3) (1,3) (2,2) (3,1) (3,0) (3,-1) (2,-2) (1,-3)
 *           (0,-3) (-1,-3) (-2,-2) (-3,-1) (-3,0) (-3,1) (-2,2) (-1,3).  For 3 <= x < W-3, 3 <= y < H-3, ring indices
 *           modulo 16: d[k] = I(x,y) - I(x+dx_k, y+dy_k); dark_k = min_{j=0..8} d[k+j], bright_k = min_{j=0..8} -d[k+j];
 *           s = max_k max(dark_k, bright_k).  The pixel is a corner iff s > t; its response is s - 1 (cornerScore's
 *           max(t, s) - 1, an integer in [t, 254]).  Every other pixel, the 3-px band along each edge included, has
 *           response 0.  A corner is kept iff its response is strictly greater than that of each of its 8 neighbours.
 *           Kept corners are listed in raster order (y, then x).  All integer.
 *   Order.  Descending response; equal responses keep raster order (the reference's std::sort leaves this open).
 *   Ssc     over the n corners in that order.  n = 0: no keys.  n = 1: that corner is the result, no search (the
 *           reference divides by zero for both).  Otherwise K = min(num_features, n) and, as written at :457-467,
 *           exp1 = H + W + 2K (int); exp2 = 4W + 4K + 4HK + H*H + W*W - 2HW + 4HWK (64-bit int);
 *           exp3 = sqrt((double)exp2); exp4 = K - 1; sol1 = -round((exp1 + exp3) / exp4),
 *           sol2 = -round((exp1 - exp3) / exp4) in fp64, round half away from zero; high = (int)max(sol1, sol2),
 *           truncated; low = (int)floor(sqrt((double)(n / K))) with the integer quotient n / K (equal to the
 *           reference's real quotient, as floor(sqrt(q)) = floor(sqrt(floor(q)))).  With Kf = (float)K:
 *           Kmin = (unsigned)round(Kf - Kf*tol), Kmax = (unsigned)round(Kf + Kf*tol), the product and the sum each
 *           rounded in float, not fused.  Then the loop of :478-523: width = low + (high - low) / 2; stop if width
 *           equals the previous width or low > high, the result being that of the last width evaluated (empty if
 *           none was); evaluate; count in [Kmin, Kmax]: stop with this result; count < Kmin: high = width - 1;
 *           else low = width + 1.
 *           One evaluation at width w >= 1: the cell of a corner is (2y div w, 2x div w) in a grid of
 *           (2H div w + 1) x (2W div w + 1) cells; in order, a corner is taken iff no corner taken before it has a
 *           cell within Chebyshev distance 2 of its own.  (These integer forms equal the reference's
 *           floor(y / (w / 2.0)): an exact quotient that is no integer lies at least 1/w from one; and
 *           floor(width / c) is exactly 2.)
 *   Final pass (:527-551) over the taken corners in order: drop a corner with x < 19, x > W-19, y < 19 or y > H-19
 *           (the reference's asymmetric bound: W-19 and H-19 themselves are kept); then drop it if a corner kept
 *           before it lies within Chebyshev distance min_dist (for keys inside that border this equals the
 *           reference's occupancy image, whose xx > 0 / yy > 0 marks never touch the pixel of a key).  What is left
 *           is mvKeys: pt = (x, y), response; then angle and descriptor by the rules above.
 *   Bounds. A key may lie 18 px from the right or bottom edge, where the map branch keeps 19.  A rotated tap reaches
 *           at most 18 px and the angle's disc 15 px, so every gather stays in bounds; hs_tracer_add_keys needs 3 px.
 */
#ifndef HS_EXTRACT_H
#define HS_EXTRACT_H

#include "hs_types.h"
#include "hs_select.h"
#include "hs_trace.h"
#include "hs_undist.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hs_extractor hs_extractor;
struct hs_image; /* include/hs_image.h, which includes this header */

/* width / height: CalibData::Width / Height, each >= 39 (the interior is not empty).  capacity >= 1: the most keys
   one extract may yield.  pattern: FeatureDetector::pattern, 256 bits x 2 taps x (x, y) = 1024 values, each within
   +-13.  A violation is HS_ERR_INVALID before any device call. */
int hs_extractor_create(hs_extractor** out, int device_id, int width, int height, int capacity,
                        const int8_t pattern[1024]);
void hs_extractor_destroy(hs_extractor* e);

/* One ExtractFeatures on the caller's selection map (W*H floats, host) and cvImgL (W*H bytes, host); *n_keys
   (nullable) = mvKeys.size().  More keys than `capacity`: HS_ERR_INVALID with *n_keys = the count needed; nothing is
   truncated and the previous result stays readable. */
int hs_extractor_extract(hs_extractor* e, const float* map, const uint8_t* img8, int* n_keys);
/* The same on the map of the selector's last make_maps, read where it lies on the device.  The selector must be on
   the extractor's device and of its size (HS_ERR_INVALID) and must have made a map (HS_ERR_STATE). */
int hs_extractor_extract_selected(hs_extractor* e, hs_selector* s, const uint8_t* img8, int* n_keys);
/* The same, with cvImgL made from the camera's raw frame (w_in*h_in bytes) on the extractor's stream, as
   hs_tracker_set_frame_u8 does; the undistorter's output size must be the extractor's size. */
int hs_extractor_extract_u8(hs_extractor* e, hs_selector* s, hs_undistorter* u, const uint8_t* raw, int* n_keys);

/* The last successful extract, all nullable: *n, xy[n][2] (mvKeys[i].pt), angle[n] (mvKeys[i].angle, degrees),
   desc[n][32] (Descriptors), blurred[W*H] (ImageBlurred).  n = 0 before the first extract. */
int hs_extractor_get(hs_extractor* e, int* n, float* xy, float* angle, uint8_t* desc, uint8_t* blurred);
/* last extract: device time (ms) from the first kernel to the last (HIP events on the extractor's stream) */
int hs_extractor_last_stats(hs_extractor* e, double* ms);

/* makeNewTraces' loop: the ImmaturePoint ctor (hs_tracer_add_points) for every key of the last extract, in key order,
   on host slot `slot`, my_type 1; x / y go device to device.  *n_added (nullable) = the keys added.  The extractor
   must be on the tracer's device and of its size, the slot must hold an image and the tracer's capacity must not be
   exceeded: HS_ERR_INVALID, nothing added.  Returns without waiting for the device (hs_tracer_get_points waits). */
int hs_tracer_add_keys(hs_tracer* t, hs_extractor* e, int slot, int* n_added);

/* ---- The UseFAST = true branch ("The FAST branch, as arithmetic" above).  A fast extract follows the rules of the
   map branch's: it writes the spare result set and swaps on success; more keys than `capacity` is HS_ERR_INVALID
   with *n_keys = the count needed and the previous result, fast or not, left intact; one wait and one 4-byte read
   per call; hs_extractor_get, hs_tracer_add_keys and the flow context read its result as any other.  The detector's
   buffers are allocated by the first fast extract. */
typedef struct { int threshold, num_features, min_dist; float tolerance; } hs_fast_params;
/* minThFAST 8, IndNumFeatures 3000, EnforcedMinDist 5, tolerance 0.1f */
void hs_fast_params_default(hs_fast_params* p);
/* threshold outside [0, 254], num_features < 2, min_dist < 0, tolerance outside [0, 1) or a null pointer:
   HS_ERR_INVALID before any device call.  img8: cvImgL, W*H bytes, host. */
int hs_extractor_extract_fast(hs_extractor* e, const hs_fast_params* p, const uint8_t* img8, int* n_keys);
/* cvImgL made from the camera's raw frame, as hs_extractor_extract_u8 */
int hs_extractor_extract_fast_u8(hs_extractor* e, const hs_fast_params* p, hs_undistorter* u, const uint8_t* raw, int* n_keys);
/* cvImgL of a device image (include/hs_image.h), as hs_extractor_extract_image */
int hs_extractor_extract_fast_image(hs_extractor* e, const hs_fast_params* p, struct hs_image* im, int* n_keys);
/* last fast extract, all nullable: corners before Ssc, the width whose result was taken (-1: none evaluated),
   response[n_keys]; for the tests, corner_xy[n_corners][2] / corner_response[n_corners] in sorted order.
   HS_ERR_STATE unless the current result is a fast extract's (none yet, or a map extract came after it). */
int hs_extractor_get_fast(hs_extractor* e, int* n_corners, int* width, float* response,
                          float* corner_xy, float* corner_response);

#ifdef __cplusplus
}
#endif
#endif /* HS_EXTRACT_H */
