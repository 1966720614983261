// hs_win_kernels.hip — device side of the incremental keyframe window (hs_ba_window.cpp).
//
//   hs_k_win_gather   the structural commit (EnergyFunctional::makeIDX after insertFrame / insertPoint /
//                     insertResidual / dropResidual / removePoint / marginalizeFrame): every point of the new layout
//                     takes its device-resident state from its old position (or from the staged upload of a point
//                     inserted since the last commit), its residual slots from the old frame column of the same
//                     target (frames keep their order; removed frames' columns vanish, new ones start empty); the
//                     frames' setNewFrameEnergyTH thresholds follow their frames.  One lane per (point, slot): the
//                     [n][8] arrays move as coalesced rows.  Pure copies: a commit changes no value, only places.
//   hs_k_win_newest   the BA -> tracker hand-off (CoarseTracker::makeCoarseDepthL0's point loop,
//                     Src/CoarseTracker.cpp:110-129): the points whose residual into the newest frame is IN, in point
//                     order, as (centerProjectedTo u, v, idepth, HdiF); one workgroup, ballot prefix sums per chunk.
//   hs_k_win_last_tail  MapPoint::lastResiduals[.].second after the optimize tail (the commit carries the pairs along).
//   hs_k_win_flag     System::flagPointsForRemoval's per-point decision (hs_flag_rule.h) and its counters.
#include <hip/hip_runtime.h>

#include "hs_win_kernels.h"

__global__ __launch_bounds__(256) void hs_k_win_gather(HsWinGatherArgs a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // the thresholds follow their frames (in place: one thread)
    float old[HS_MAXF];
    for (int f = 0; f < HS_MAXF; f++) old[f] = a.frameTH[f];
    for (int f = 0; f < a.nF; f++) a.frameTH[f] = a.col_src[f] >= 0 ? old[a.col_src[f]] : a.th_init[f];
  }
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int p = gid >> 3, t = gid & 7;
  if (p >= a.n) return;
  const int src = a.src[p];
  const size_t o = (size_t)p * 8 + t;
  if (src >= 0) {
    const size_t i = (size_t)src * 8 + t;
    a.to.color[o] = a.from.color[i];
    a.to.weight[o] = a.from.weight[i];
    if (t == 0) {
      a.to.u[p] = a.from.u[src];
      a.to.v[p] = a.from.v[src];
      a.to.idepth[p] = a.from.idepth[src];
      a.to.idepth_zero[p] = a.from.idepth_zero[src];
      a.to.priorF[p] = a.from.priorF[src];
      a.to.relBL[p] = a.from.relBL[src];
      a.to.nGood[p] = a.from.nGood[src];
      a.hdif_to[p] = a.hdif_from[src];
    }
  } else {
    // a staged point: the commit blob's (hs_ba_insert_points), or the device staging array hs_k_act_stage filled
    const int k = -src - 1;
    const HsStagedPoint& s = (k & HS_WIN_SRC_DEV) ? a.staged_dev[k & ~HS_WIN_SRC_DEV] : a.staged[k];
    a.to.color[o] = s.color[t];
    a.to.weight[o] = s.weight[t];
    if (t == 0) {
      a.to.u[p] = s.u;
      a.to.v[p] = s.v;
      a.to.idepth[p] = s.idepth;
      a.to.idepth_zero[p] = s.idepth_zero;
      a.to.priorF[p] = s.priorF;
      a.to.relBL[p] = s.relBL;
      a.to.nGood[p] = s.nGood;
      a.hdif_to[p] = 0.f;
    }
  }
  // residual slot t: a committed residual keeps its state and centre projection (old column of the same frame), a new
  // one starts in the given state, a slot without a residual is OOB
  const unsigned code = a.newres[o];
  uint8_t st = HS_RES_OOB;
  float c0 = 0.f, c1 = 0.f, c2 = 0.f;
  if (code == HS_WIN_KEEP) {
    const size_t i = (size_t)src * 8 + a.col_src[t];
    st = a.from.r_state[i];
    c0 = a.from.r_center[3 * i]; c1 = a.from.r_center[3 * i + 1]; c2 = a.from.r_center[3 * i + 2];
  } else if (code != HS_WIN_NONE) {
    st = (uint8_t)code;
  }
  a.to.r_state[o] = st;
  a.to.r_center[3 * o] = c0;
  a.to.r_center[3 * o + 1] = c1;
  a.to.r_center[3 * o + 2] = c2;
  // lastResiduals slot t: the state an old slot holds, or a literal one; its tail column for the new layout
  if (t < 2) {
    const unsigned lc = a.lastc[(size_t)p * 4 + t];
    uint8_t ls = (uint8_t)(lc & 3u);
    if ((lc & HS_WIN_LAST_KEEP) && src >= 0) ls = a.from.last[(size_t)src * 2 + (lc & 1u)];
    a.to.last[(size_t)p * 2 + t] = ls;
    a.last_tgt[(size_t)p * 2 + t] = (int8_t)a.lastc[(size_t)p * 4 + 2 + t];
  }
}

// The optimize tail's lastResiduals update (System::linearizeAll(true), Src/FullSystemOptimize.cpp:128-135): a slot
// whose residual is still in the window takes that residual's state.  One lane per (point, slot).
__global__ __launch_bounds__(256) void hs_k_win_last_tail(int n, const int8_t* __restrict__ last_tgt,
                                                          const uint8_t* __restrict__ r_state,
                                                          uint8_t* __restrict__ last) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * n) return;
  const int t = last_tgt[i];
  if (t >= 0 && t < HS_MAXF) last[i] = r_state[(size_t)(i >> 1) * 8 + t];
}

// System::flagPointsForRemoval (Src/Mapping.cpp:248-328): one lane per point applies hs::flag_rule to the point's
// device-resident state.  The residual list and the slot states are one 8-byte row each.  Every lane stays for the
// ballots; the counters are integers, so the order of the waves' atomics does not matter.
__global__ __launch_bounds__(256) void hs_k_win_flag(HsWinFlagArgs a) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  int code = -1;
  if (p < a.n) {
    const unsigned long long ord = reinterpret_cast<const unsigned long long*>(a.res_order)[p];
    const unsigned long long st = reinterpret_cast<const unsigned long long*>(a.r_state)[p];
    int nres = 0, vis = 0;
    for (int q = 0; q < 8; q++) {
      const int t = (int)(int8_t)(ord >> (8 * q));
      if (t < 0 || t >= HS_MAXF) break;
      nres++;
      if (((a.marg_mask >> t) & 1u) && (uint8_t)(st >> (8 * t)) == HS_RES_IN) vis++;
    }
    const unsigned l = reinterpret_cast<const unsigned short*>(a.last)[p];
    const int h = a.pt_host[p];
    const bool host_flagged = h >= 0 && h < HS_MAXF && ((a.marg_mask >> h) & 1u);
    code = hs::flag_rule(nres, vis, a.nGood[p], a.idepth[p], a.hdif[p], (int)(l & 0xffu), (int)(l >> 8), host_flagged);
    const int act = code & hs::HS_FLAG_ACTION;
    a.action[p] = (uint8_t)act;
    a.marg[p] = act == hs::HS_FLAG_MARG ? 1 : 0;
  }
  const bool on = code >= 0;
  const bool bit[6] = {on && (code & hs::HS_FLAG_NORES), on && (code & hs::HS_FLAG_OOB), on && (code & hs::HS_FLAG_IN),
                       on && (code & hs::HS_FLAG_ININ), on && (code & hs::HS_FLAG_ACTION) == hs::HS_FLAG_DROP,
                       on && (code & hs::HS_FLAG_ACTION) == hs::HS_FLAG_MARG};
  for (int k = 0; k < 6; k++) {
    const int cnt = __popcll(__ballot(bit[k]));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&a.counts[k], cnt);
  }
}

// points p (in order) with res_of_slot[p][newest] >= 0 and state IN -> out[cap * {0,1,2,3}] = cu, cv, cid, HdiF
__global__ __launch_bounds__(1024) void hs_k_win_newest(int n, int newest, const int* __restrict__ res_of_slot,
                                                        const uint8_t* __restrict__ r_state,
                                                        const float* __restrict__ r_center,
                                                        const float* __restrict__ hdif, float* __restrict__ out,
                                                        int cap, int* __restrict__ n_out) {
  __shared__ int wsum[16];
  __shared__ int base_s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int c0 = 0; c0 < n; c0 += 1024) {
    const int p = c0 + tid;
    bool take = false;
    if (p < n) {
      const size_t sl = (size_t)p * 8 + newest;
      take = res_of_slot[sl] >= 0 && r_state[sl] == HS_RES_IN;
    }
    const unsigned long long m = __ballot(take);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    int off = base_s;
    for (int w = 0; w < wv; w++) off += wsum[w];
    if (take) {
      const int q = off + before;
      const size_t sl = (size_t)p * 8 + newest;
      out[q] = r_center[3 * sl];
      out[cap + q] = r_center[3 * sl + 1];
      out[2 * cap + q] = r_center[3 * sl + 2];
      out[3 * cap + q] = hdif[p];
    }
    __syncthreads();
    if (tid == 0) {
      int s = 0;
      for (int w = 0; w < 16; w++) s += wsum[w];
      base_s += s;
    }
    __syncthreads();
  }
  if (tid == 0) *n_out = base_s;
}
