// hs_flow_kernels.h — kernels of include/hs_flow.h: the padded u8 pyramid, its Scharr derivative and the
// wave-per-point pyramidal Lucas-Kanade tracker.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int kFlowWin = 15;        // the window's side
constexpr int kFlowPad = 15;        // border of every stored level: no window tap lies further outside
constexpr int kFlowMaxLevels = 3;   // maxLevel 2
constexpr int kFlowIters = 30;

// One frame's levels in one allocation each: level l is a (w[l] + 30) x (h[l] + 30) array at element `off[l]` of
// the image buffer (u8, border reflected) and of the derivative buffer (short2 (dx, dy), border zero).
struct HsFlowLevels {
  int n;
  int w[kFlowMaxLevels], h[kFlowMaxLevels];
  int off[kFlowMaxLevels];
};

// level 0 with its border from a plain W x H image
struct HsFlowPadArgs {
  int w, h;
  const uint8_t* src;  // w * h
  uint8_t* dst;        // (w + 30) * (h + 30)
};

// pyrDown of a padded level into the next padded level, border included
struct HsFlowDownArgs {
  int sw, sh, dw, dh;
  const uint8_t* src;  // (sw + 30) * (sh + 30)
  uint8_t* dst;        // (dw + 30) * (dh + 30)
};

struct HsFlowScharrArgs {
  int w, h;
  const uint8_t* img;  // (w + 30) * (h + 30)
  short2* deriv;       // the same shape; zero outside the level
};

struct HsFlowLkArgs {
  HsFlowLevels lv;
  const uint8_t* prev_img;
  const short2* prev_deriv;
  const uint8_t* next_img;
  int n;
  const float2* prev_xy;
  const float2* init_xy;  // nullable: no guess
  float2* xy;
  uint8_t* status;
  float* err;
  uint8_t* good;  // status && err < max_l1_error
  float max_l1_error;
  int* n_good;                  // += the good points
  unsigned long long* n_iters;  // += the iterations run
};

// the extractor's separate x / y arrays as the (x, y) pairs the tracker reads
__global__ void hs_k_flow_pack_xy(int n, const float* x, const float* y, float2* xy);
__global__ void hs_k_flow_pad(HsFlowPadArgs a);
__global__ void hs_k_flow_pyrdown(HsFlowDownArgs a);
__global__ void hs_k_flow_scharr(HsFlowScharrArgs a);
__global__ void hs_k_flow_lk(HsFlowLkArgs a);

// ComputeMeanOpticalFlow(MatchedPtsBkp, MatchedPts) over the good points
struct HsFlowMeanArgs {
  int n;
  const float2 *prev_xy, *xy;
  const uint8_t* good;
  float* mean;  // one float
};
__global__ void hs_k_flow_mean(HsFlowMeanArgs a);  // 1 block of 256

// FirstFramePts (= mvKeys[i].pt, n pairs) where the last hs_flow_set_first* left them on the device; false before
// the first one.  Every hs_flow entry waits for its own work before it returns, so the pairs are complete; only the
// next hs_flow_set_first* rewrites them, so a consumer waits for its own reads before it returns
// (hs_refiner_set_points_flow does, for its violation count).
struct hs_flow;
bool hs_flow_first_points(hs_flow* f, int* device, int* W, int* H, int* n, const float2** d_first);

// FirstFramePts, MatchedPts and MatchedStatus (n each) where the last hs_flow_track* left them on the device, for the
// two-view fit (hs_twoview_fit_flow); false before the first frame.  first_id counts the hs_flow_set_first* calls, so a
// consumer can tell whether two reads belong to one first frame.  `stream` is the flow's: a consumer on another stream
// orders itself behind the last track with an event recorded there.  Only the next hs_flow_set_first* / _track*
// rewrites the arrays, so a consumer waits for its own reads before it returns.
struct HsFlowKeys {
  int device, n;
  long long first_id;
  bool tracked;
  const float2 *first, *matched;
  const uint8_t* good;
  hipStream_t stream;
};
bool hs_flow_tracked_keys(hs_flow* f, HsFlowKeys* k);
