// hs_win_kernels.h — argument blocks of the incremental-window kernels (hs_win_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hs_types.h"
#include "hs_flag_rule.h"
#include "hs_layout.h"

// slot codes of a commit's residual table [n][8]
constexpr unsigned HS_WIN_KEEP = 0xFF;  // a committed residual: state / centre from the old column of its frame
constexpr unsigned HS_WIN_NONE = 0xFE;  // no residual in this slot
// (any other value: a residual inserted since the last commit, starting in that ResState)
// codes of a commit's lastResiduals table [n][4] = (code of slot 0, of slot 1, tail column of slot 0, of slot 1): a code
// is a literal ResState, or HS_WIN_LAST_KEEP | s: the state the point's old slot s holds on the device; a tail column
// is the window frame whose residual state the optimize tail copies into the slot, (int8) -1 when that residual is gone
constexpr unsigned HS_WIN_LAST_KEEP = 0x10;

// a staged point's src is -(1 + k); k carries this bit when the point lies in the context's device staging array
// (written by hs_tracer_activate_ba's hs_k_act_stage) and not in the commit blob
constexpr int HS_WIN_SRC_DEV = 1 << 30;

// a point inserted since the last commit (uploaded with the commit's structure, or staged on the device)
struct HsStagedPoint {
  float u, v, idepth, idepth_zero, priorF, relBL;
  int nGood;
  float color[8], weight[8];
};

struct HsWinPointSet {
  float *u, *v, *idepth, *idepth_zero, *priorF, *color, *weight, *relBL;
  int* nGood;
  uint8_t* r_state;
  float* r_center;
  uint8_t* last;  // [n][2] lastResiduals[.].second
};

struct HsWinGatherArgs {
  int n;                        // points of the new layout
  int nF;                       // frames of the new layout
  int col_src[HS_MAXF];         // new frame column -> old column (-1: inserted since the last commit)
  float th_init[HS_MAXF];       // frameEnergyTH of the inserted frames
  const int* src;               // [n] old position, or -(1 + k) for staged point k (k | HS_WIN_SRC_DEV: of staged_dev)
  const uint8_t* newres;        // [n][8] slot codes
  const HsStagedPoint* staged;
  const HsStagedPoint* staged_dev;  // the context's device staging array (hs_ctx::d_act_stage)
  HsWinPointSet from, to;
  const float* hdif_from;       // the last solve's HdiF (old layout)
  float* hdif_to;
  float* frameTH;               // [HS_MAXF] permuted in place
  const uint8_t* lastc;         // [n][4] lastResiduals codes and tail columns (above)
  int8_t* last_tgt;             // [n][2] the tail columns, written for the new layout
};

// hs_k_win_flag: System::flagPointsForRemoval's decisions over the committed window
struct HsWinFlagArgs {
  int n;
  unsigned marg_mask;           // bit f: window frame f is FlaggedForMarginalization
  const float* idepth;
  const int* nGood;
  const float* hdif;            // the last solve's HdiF
  const int* pt_host;
  const uint8_t* r_state;       // [n][8], slot layout
  const int8_t* res_order;      // [n][8] residual lists (targets, -1 terminated)
  const uint8_t* last;          // [n][2]
  uint8_t* action;              // [n] 0 keep, 1 drop, 2 marginalize
  uint8_t* marg;                // [n] the marginalization pass's flags (action == 2)
  int* counts;                  // [6] flag_nores, flag_oob, flag_in, flag_inin, n_drop, n_marg (zero on entry)
};

__global__ void hs_k_win_gather(HsWinGatherArgs a);
__global__ void hs_k_win_newest(int n, int newest, const int* res_of_slot, const uint8_t* r_state,
                                const float* r_center, const float* hdif, float* out, int cap, int* n_out);
__global__ void hs_k_win_last_tail(int n, const int8_t* last_tgt, const uint8_t* r_state, uint8_t* last);
__global__ void hs_k_win_flag(HsWinFlagArgs a);
