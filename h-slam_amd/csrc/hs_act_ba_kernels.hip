// hs_act_ba_kernels.hip — device side of hs_tracer_activate_ba (hs_trace.cpp): point activation whose window is a BA
// context's.
//
//   hs_k_act_form     activatePointsMT's per-frame KRKi / Kt (Src/Mapping.cpp:366-369) and the pairs' PRE_RTll /
//                     PRE_tTll / PRE_aff_mode (FrameFramePrecalc::set) from the frames of the BA's device state: one
//                     thread per (host, target) pair, the diagonal threads also their frame.  The arithmetic is
//                     hs_host_math.h's make_act_*, the same inlines hs_debug_act_inputs runs on the host.
//   hs_k_trc_form     traceNewCoarse's per-host KRKi / Kt / aff (Src/Mapping.cpp:500-513) of hs_tracer_trace_ba: one
//                     thread per window frame at its committed index, against the new frame's pose / affine pair /
//                     exposure (by value), into the tracer's host table at the frame's slot.  hs_host_math.h's
//                     make_trace_host, the inline hs_debug_trace_hosts runs on the host.
//   hs_k_act_stage    the activated points as HsStagedPoint records in toOptimize order (the hs_k_win_gather's second
//                     staged source).  One workgroup: ballot prefix sums per chunk of the list give every activated
//                     entry its rank (no atomics: the order is the list's), then one lane per (point, pattern slot)
//                     writes the rows.
//   hs_k_cmp_*        stable compaction of the tracer's per-point arrays: keep flags and their exclusive scan inside
//                     each block of HS_CMP_NT points, an exclusive scan of the blocks' totals by one workgroup, and a
//                     scatter of every array into the second buffer set (one lane per (point, component)).
#include <hip/hip_runtime.h>

#include "hs_imm_ctor.h"
#include "hs_kernels.h"
#include "hs_trace_kernels.h"
#include "hs_win_kernels.h"

__global__ __launch_bounds__(64) void hs_k_act_form(HsActFormArgs a) {
  const int i = threadIdx.x;
  const int nF = a.nF;
  if (i >= nF * nF) return;
  const int h = i / nF, t = i - h * nF;
  hs_act_pair& p = a.pairs[i];
  hs::make_act_pair(a.st->frames[h], a.st->frames[t], p.RTll, p.tTll, p.aff);
  if (h == t) {
    hs_act_frame& f = a.frames[h];
    f.slot = a.slot[h];
    f.flagged_for_marg = a.flagged[h];
    float K1[9], Ki0[9];
    hs::make_act_K(a.st->calib, K1, Ki0);
    hs::make_act_frame(a.st->frames[h], a.st->frames[nF - 1], K1, Ki0, f.KRKi, f.Kt);
  }
}

__global__ __launch_bounds__(64) void hs_k_trc_form(HsTrcFormArgs a) {
  const int f = threadIdx.x;
  if (f >= a.nF) return;
  const hs::SE3 nw = hs::SE3::fromData(a.new_worldToCam);
  hs::make_trace_host(a.st->frames[a.idx[f]], nw, a.new_exposure, a.new_aff[0], a.new_aff[1], a.st->calib,
                      &a.hosts[a.slot[f]]);
}

using hs_imm::block_rank;

__global__ __launch_bounds__(1024) void hs_k_act_stage(HsActStageArgs a) {
  __shared__ int wsum[16];
  const int tid = threadIdx.x;
  int base = 0;
  for (int c0 = 0; c0 < a.n; c0 += 1024) {  // uniform trip count: every thread reaches the barriers
    const int k = c0 + tid;
    const bool take = k < a.n && a.action[a.toopt[k]] == HS_ACT_ACTIVATED;
    int total;
    const int r = block_rank(take, wsum, &total);
    if (k < a.n) a.pos[k] = take ? base + r : -1;
    base += total;
  }
  __syncthreads();  // pos[] of this workgroup's own stores
  for (int j = tid; j < a.n * 8; j += 1024) {
    const int k = j >> 3, q = j & 7;
    const int r = a.pos[k];
    if (r < 0) continue;
    const int i = a.toopt[k];
    HsStagedPoint& s = a.out[a.base + r];
    s.color[q] = a.color[(size_t)i * 8 + q];
    s.weight[q] = a.weights[(size_t)i * 8 + q];
    if (q == 0) {
      // the new MapPoint (Include/MapPoint.h:92-115, Src/FullSystemOptPoint.cpp:142-148): idepth = idepth_zero = the
      // optimised idepth, no depth prior, maxRelBaseline 0, numGoodResiduals 0
      const float id = a.idepth[i];
      s.u = a.u[i];
      s.v = a.v[i];
      s.idepth = id;
      s.idepth_zero = id;
      s.priorF = 0.f;
      s.relBL = 0.f;
      s.nGood = 0;
    }
  }
}

__global__ __launch_bounds__(HS_CMP_NT) void hs_k_cmp_flags(HsCmpArgs a) {
  __shared__ int wsum[HS_CMP_NT / 64];
  const int i = blockIdx.x * HS_CMP_NT + threadIdx.x;
  bool keep = false;
  if (i < a.n) {
    keep = a.keep_in ? a.keep_in[i] != 0 : a.action[i] == HS_ACT_KEEP;
    if (a.drop_slot) {
      const int h = a.from.host[i];
      if (h >= 0 && h < HS_TRC_MAXHOST && a.drop_slot[h]) keep = false;
    }
  }
  int total;
  const int r = block_rank(keep, wsum, &total);
  if (i < a.n) a.pos[i] = keep ? r : -1;
  if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
}

// blk[b] -> the number of kept points in the blocks before b
__global__ __launch_bounds__(1024) void hs_k_cmp_scan(HsCmpArgs a, int nblk) {
  __shared__ int wtot[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int base = 0;
  for (int c0 = 0; c0 < nblk; c0 += 1024) {
    const int b = c0 + tid;
    const int v = b < nblk ? a.blk[b] : 0;
    int inc = v;  // inclusive scan inside the wave
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wtot[wv] = inc;
    __syncthreads();
    int off = 0, all = 0;
    for (int w = 0; w < 16; w++) {
      const int s = wtot[w];
      off += w < wv ? s : 0;
      all += s;
    }
    __syncthreads();
    if (b < nblk) a.blk[b] = base + off + inc - v;
    base += all;
  }
}

__global__ __launch_bounds__(256) void hs_k_cmp_scatter(HsCmpArgs a) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = gid >> 3, q = gid & 7;
  if (i >= a.n) return;
  const int r = a.pos[i];
  if (r < 0) return;
  const size_t s = i, d = (size_t)a.blk[i / HS_CMP_NT] + r;
  a.to.color[d * 8 + q] = a.from.color[s * 8 + q];
  a.to.weights[d * 8 + q] = a.from.weights[s * 8 + q];
  if (q < 4) a.to.gradH[d * 4 + q] = a.from.gradH[s * 4 + q];
  if (q < 2) a.to.uv[d * 2 + q] = a.from.uv[s * 2 + q];
  if (q == 0) {
    a.to.host[d] = a.from.host[s];
    a.to.u[d] = a.from.u[s];
    a.to.v[d] = a.from.v[s];
    a.to.energyTH[d] = a.from.energyTH[s];
    a.to.quality[d] = a.from.quality[s];
    a.to.idmin[d] = a.from.idmin[s];
    a.to.idmax[d] = a.from.idmax[s];
    a.to.interval[d] = a.from.interval[s];
    a.to.status[d] = a.from.status[s];
    a.to.steps[d] = a.from.steps[s];
    a.to.type[d] = a.from.type[s];
  }
}
