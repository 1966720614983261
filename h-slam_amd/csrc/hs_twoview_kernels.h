// hs_twoview_kernels.h — kernels of include/hs_twoview.h: the two-view fit as eight small launches on one stream.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/hs_twoview.h"

constexpr int kTvMaxSets = HS_TWOVIEW_MAX_SETS;
constexpr int kTvMaxRt = 8;

// what the launches of one fit hand to each other, and the record the host reads back
struct HsTvState {
  int bad;                 // 1: a set points at a key with status 0; 2: fewer than 8 matched keys to draw from.  Every
                           // later kernel of the fit returns at once
  int m;                   // hs_k_tv_good_list: the keys with status != 0
  int best_h, best_f;      // the winners (-1: no score above 0)
  float SH, SF;
  int n_in_h, n_in_f;      // the winners' inliers (integer atomics)
  int model, n_rt, why;    // hs_k_tv_decompose: why 0, 1 or 2
  float rt[kTvMaxRt][12];  // R (9, row-major), t (3)
  int n_good[kTvMaxRt];
  float parallax[kTvMaxRt];
  hs_twoview_result res;
};

struct HsTvArgs {
  int n, ns_h, ns_f;
  int n_in_sets;  // the sets at in_sets (0: none, the debug entries)
  float fx, fy, cx, cy;
  HsTvState* st;
  // a fit's inputs where the caller left them
  const float2 *in1, *in2;
  const uint8_t* in_status;
  const int* in_sets;
  // the fit's state
  float4* keys;     // (u1, v1, u2, v2)
  uint8_t* status;
  int* sets;        // [ns][8]
  float* norm;      // meanX, meanY, sX, sY of image 1, then of image 2
  float* models;    // [ns_h][9] H21, then at 9 * kTvMaxSets [ns_f][9] F21
  float* h12;       // [ns_h][9]
  float* scores;    // [ns_h], then at kTvMaxSets [ns_f]
  uint8_t* inl;     // [2][n]: the winners' masks
  const uint8_t* rt_inl;  // the mask hs_k_tv_check_rt reads; null: the chosen model's
  float* rt_p3d;    // [8][n][3]
  float* rt_cos;    // [8][n]
  uint8_t* rt_pass; // [8][n]
  uint8_t* rt_good; // [8][n]
  uint8_t* tri;     // [n]
  float* z;         // [n]
  float* p3d;       // [n][3]
  // the draw of the sets (hs_k_tv_good_list, hs_k_tv_draw)
  int n_draw;            // the sets to draw (0: the sets are the caller's)
  int* all;              // [n]: the keys with in_status != 0, ascending
  const uint32_t* words; // [8 * n_draw]: the generator's next() values in order
  int* draw_out;         // [n_draw][8]
};

__global__ void hs_k_tv_begin(HsTvArgs a);      // 1 block: the status rule of the sets, the counters' reset
__global__ void hs_k_tv_good_list(HsTvArgs a);  // 1 block of 1024: the stable compaction of in_status != 0, and m
__global__ void hs_k_tv_draw(HsTvArgs a);       // one lane per set: the swap-and-pop over `all`
__global__ void hs_k_tv_pack(HsTvArgs a);       // n threads: keys, status, sets into the state
__global__ void hs_k_tv_normalize(HsTvArgs a);  // 2 blocks: one per image
__global__ void hs_k_tv_hypotheses(HsTvArgs a); // one wave per (set, model): ns_h + ns_f blocks of 64
__global__ void hs_k_tv_scores(HsTvArgs a);     // one block per (set, model)
__global__ void hs_k_tv_winners(HsTvArgs a);    // n threads: both argmax, both masks
__global__ void hs_k_tv_decompose(HsTvArgs a);  // one lane
__global__ void hs_k_tv_check_rt(HsTvArgs a);   // one lane per (motion hypothesis, match): grid (ceil(n / 256), 8)
__global__ void hs_k_tv_select(HsTvArgs a);     // one block per motion hypothesis
__global__ void hs_k_tv_finish(HsTvArgs a);     // 1 block

// the last successful fit's vbTriangulated and mvIniP3D[i].z / median_depth on the device, for
// hs_refiner_set_points_twoview; false when the last fit did not succeed or was not a fit from `flow`'s current first
// frame and key count.  The fit has waited for its kernels, so the arrays are complete.
struct hs_twoview;
struct hs_flow;
bool hs_twoview_triangulated(hs_twoview* tv, hs_flow* flow, int* device, int* n, const uint8_t** d_tri,
                             const float** d_z);
