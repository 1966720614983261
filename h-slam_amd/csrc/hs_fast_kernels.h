// hs_fast_kernels.h — kernels of the UseFAST branch of include/hs_extract.h: the corner response plane, strict 3x3
// suppression with ordered compaction, the stable sort by response, Ssc and the final pass.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int kFastRing = 3;                          // the ring's radius: responses are 0 within 3 px of an edge
constexpr int kFastTileW = 64, kFastTileH = 16;       // one 256-thread block of hs_k_fast_resp, 4 rows per thread
constexpr int kFastInfoCorners = 0, kFastInfoWidth = 1, kFastInfoTaken = 2, kFastInfoLow = 3, kFastInfoHigh = 4,
              kFastInfoSize = 5;  // HsFastArgs::info

struct HsFastArgs {
  int W, H;
  int threshold, num_features, min_dist, cap;  // cap: entries of x / y / response
  float tolerance;
  const uint8_t* img;  // W*H cvImgL
  uint8_t* resp;       // W*H response plane (0: no corner)
  int* row_cnt;        // [H - 6] kept corners per row
  int* c_idx;          // [max corners] raster index y*W + x, raster order
  uint8_t* c_resp;     // [max corners]
  int* s_idx;          // the same, sorted by descending response, ties in raster order
  uint8_t* s_resp;
  int max_high;        // widths 1 .. max_high have a workgroup, a covered grid and a taken list (hs_fast_width_tables)
  const size_t* woff;  // [max_high] byte offset of width w's covered grid in `covered` (at woff[w - 1]), 16-aligned
  const size_t* toff;  // [max_high] entry offset of width w's taken list in `wtaken`
  uint8_t* covered;    // one byte per cell, (2H div w + 1) * (2W div w + 1) cells for width w, padded to 16
  int* wtaken;         // per width: the sorted indices it took, in order
  int* wcnt;           // [max_high] corners taken per evaluated width
  uint8_t* occ;        // W*H, zero on entry to hs_k_fast_final: pixels within min_dist of a kept key
  int* info;           // [5] corners, the width whose result was taken (-1: none), corners taken, low, high
  float* x;            // [cap] mvKeys
  float* y;
  float* response;
  int* count;          // mvKeys.size() (also when > cap: the entries beyond cap are not written)
};

__global__ void hs_k_fast_resp(HsFastArgs a);
__global__ void hs_k_fast_count(HsFastArgs a);
__global__ void hs_k_fast_write(HsFastArgs a);
__global__ void hs_k_fast_sort(HsFastArgs a);
__global__ void hs_k_fast_ssc(HsFastArgs a);
__global__ void hs_k_fast_final(HsFastArgs a);
