// hs_map_kernels.h — argument blocks of the point map's kernels (hs_map_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hs_map.h"
#include "hs_frame_rule.h"
#include "hs_kernels.h"
#include "hs_layout.h"

static_assert(sizeof(hs_map_record) == 64, "hs_k_map_retire stores a record as four 16-byte quarters");

constexpr int HS_MAP_CLOUD_NT = 1024;               // hs_k_map_cloud: one workgroup, lane = (point, pattern pixel)
constexpr int HS_MAP_CLOUD_PTS = HS_MAP_CLOUD_NT / 8;  // points per compaction chunk

// hs_k_map_rank: the committed positions of the action != 0 points, in window order (stable compaction, one workgroup)
// list[q] is written only for q < cap; n_out (nullable) receives the count
__global__ void hs_k_map_rank(int n, const uint8_t* action, int* list, int cap, int* n_out);

// hs_k_map_retire: record first + i <- the window state of the point at committed position list[i]
struct HsMapRetireArgs {
  int n;                       // points to retire
  const int* list;             // [n] committed positions
  const int* handle;           // [n] their handles (the window's device state does not hold them; host-mapped)
  const uint8_t* action;       // [nP] hs_k_win_flag's decisions (1 -> OUTLIER, 2 -> MARGINALIZED), or nullptr:
  const uint8_t* status;       // [n] the status of each (host-mapped)
  int frame_id[HS_MAXF];       // window frame -> hs_frame.id
  const int* pt_host;
  const float *u, *v, *idepth, *idepth_zero, *hdif, *relBL, *color;
  const int* nGood;
  hs_map_record* rec;          // the store, at the first new record
};
__global__ void hs_k_map_retire(HsMapRetireArgs a);

// hs_k_map_cloud: KFDisplay::RefreshPC for one keyframe
struct HsMapCloudArgs {
  int act_begin, act_n;        // the frame's active points: committed positions [act_begin, act_begin + act_n)
  const float *u, *v, *idepth, *hdif, *relBL;
  const HsDevState* st;        // the window's calibration
  int n_runs;                  // the frame's record runs
  const int* runs;             // [n_runs][2] (first record, candidates before the run); [n_runs][1] = all candidates
  const hs_map_record* rec;
  float* xyz;                  // [cap_pts * 8][3]
  uint8_t* rgb;                // [cap_pts * 8][3]
  int cap_pts;
  int* out;                    // [0] vertices, [1..4] the bits of fxi, fyi, cxi, cyi
};
__global__ void hs_k_map_cloud(HsMapCloudArgs a);

// hs_k_win_flag_frames: the affine factors and pair distances from the device-resident frame state, then hs::frame_rule
struct HsFlagFramesArgs {
  int nF;
  const HsDevState* st;
  int in[HS_MAXF], out[HS_MAXF], kf_id[HS_MAXF];
  hs_frame_marg_params P;
  uint8_t* flagged;            // [HS_MAXF]
};
__global__ void hs_k_win_flag_frames(HsFlagFramesArgs a);
