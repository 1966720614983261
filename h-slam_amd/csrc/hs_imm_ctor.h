// hs_imm_ctor.h — the per-point body of the ImmaturePoint constructor (Src/ImmaturePoint.cpp:7-32), shared by
// hs_k_imm_ctor (hs_trace_kernels.hip) and hs_k_init_seed (hs_init_kernels.hip) so the arithmetic cannot drift, and
// the rank of a flagged thread among its workgroup's (the stable compactions of hs_act_ba_kernels.hip and
// hs_init_kernels.hip).  Include inside a file compiled with `#pragma clang fp contract(off)`.
#pragma once
#include <hip/hip_runtime.h>

#include "hs_interp.h"

#pragma clang fp contract(off)

namespace hs_imm {

// the residual pattern (patternP, Include/Settings.h: pattern 8)
constexpr int kPat[8][2] = {{0, -2}, {-1, -1}, {1, -1}, {-2, 0}, {0, 0}, {2, 0}, {-1, 1}, {0, 2}};

// 8 BiLin taps of the host frame around (u, v): color, weights and gradH = sum of (dx, dy)(dx, dy)^T in pattern
// order.  Returns false when a colour is not finite (the reference sets energyTH = NaN and returns): the colours
// up to and including it stand, the later ones are 0, every weight from it on is 0 and gradH holds the sums so far.
__device__ __forceinline__ bool ctor_point(const float4* __restrict__ img, float u, float v, int W, int H,
                                           float outlierTHSumComponent, float col[8], float wgt[8], float g[4]) {
  float g0 = 0, g1 = 0, g2 = 0, g3 = 0;
  bool bad = false;
  // all 8 taps first: their 32 loads are in flight together, not one tap's behind the previous tap's branches
  float3 tap[8];
#pragma unroll
  for (int idx = 0; idx < 8; idx++) tap[idx] = hs_img::interp33BiLin(img, u + kPat[idx][0], v + kPat[idx][1], W, H);
#pragma unroll
  for (int idx = 0; idx < 8; idx++) {
    const float3 ptc = tap[idx];
    col[idx] = bad ? 0.f : ptc.x;
    wgt[idx] = 0;
    if (bad) continue;
    if (!isfinite(ptc.x)) {
      bad = true;
      continue;
    }
    g0 = g0 + ptc.y * ptc.y;
    g1 = g1 + ptc.y * ptc.z;
    g2 = g2 + ptc.z * ptc.y;
    g3 = g3 + ptc.z * ptc.z;
    wgt[idx] = sqrtf(outlierTHSumComponent / (outlierTHSumComponent + (ptc.y * ptc.y + ptc.z * ptc.z)));
  }
  g[0] = g0;
  g[1] = g1;
  g[2] = g2;
  g[3] = g3;
  return !bad;
}

// exclusive prefix of `take` over the workgroup's threads in thread order; *total = the workgroup's count.
// wsum: one int per wave (shared).  Ends with a barrier, so wsum may be reused at once.
__device__ __forceinline__ int block_rank(bool take, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  const unsigned long long m = __ballot(take);
  if (lane == 0) wsum[wv] = __popcll(m);
  __syncthreads();
  int off = 0, all = 0;
  for (int w = 0; w < nw; w++) {
    const int s = wsum[w];
    off += w < wv ? s : 0;
    all += s;
  }
  __syncthreads();
  *total = all;
  return off + __popcll(m & ((1ull << lane) - 1ull));
}

}  // namespace hs_imm
