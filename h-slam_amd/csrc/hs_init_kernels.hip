// hs_init_kernels.hip — device side of the initializer hand-off (include/hs_init.h, hs_refine.cpp).
//
//   hs_k_ref_points   DirectRefinement's Pnt set-up (Src/Initializer.cpp:1362-1382) from the flow context's
//                     FirstFramePts: one thread per key writes its entry of every plane of the refiner's state block
//                     (consecutive threads, consecutive floats of a plane) and counts the keys outside the image.
//                     invz = (float)(1.0 / (double)z): the host's fp64 divide, correctly rounded on both sides.
//   hs_k_init_seed    System::InitFromInitializer's point loop (Src/System.cpp:265-290): per key the videpth and the
//                     decision of hs_init_rule.h, the ImmaturePoint constructor (hs_imm_ctor.h, the body hs_k_imm_ctor
//                     runs) at (u + 0.5, v + 0.5) on the first frame, and the new MapPoint as one HsStagedPoint.  One
//                     workgroup: ballot prefix sums per sweep of 1024 keys give every seeded key its rank (no atomics:
//                     the order is mvKeys'), and the thread that ran the constructor writes the record.
#include <hip/hip_runtime.h>

#include "hs_init_kernels.h"
#include "hs_init_rule.h"

#pragma clang fp contract(off)
#include "hs_imm_ctor.h"

__global__ __launch_bounds__(256) void hs_k_ref_points(HsRefPointsArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const size_t n = (size_t)a.n;
  const float2 k = a.first[i];
  // hs_refiner_set_points' range rule
  if (!isfinite(k.x) || !isfinite(k.y) || k.x < 0 || k.y < 0 || k.x > a.W - 1 || k.y > a.H - 1) atomicAdd(a.n_bad, 1);
  const bool tri = a.tri[i] != 0;
  const float invz = tri ? (float)(1.0 / (double)a.z[i]) : 1.0f;
  for (int p = 0; p < a.n_planes; p++) {
    float x = 0.f;
    if (p == a.pl_u) x = k.x;
    else if (p == a.pl_v) x = k.y;
    else if (p == a.pl_invz || p == a.pl_id || p == a.pl_idn || p == a.pl_ir) x = invz;
    a.pf[(size_t)p * n + i] = x;
  }
  a.pb[i] = tri ? 1 : 0;
  a.pb[n + i] = 1;  // isGood
  a.pb[2 * n + i] = 0;
}

__global__ __launch_bounds__(1024) void hs_k_init_seed(HsInitSeedArgs a) {
  __shared__ int wsum[16];
  const int tid = threadIdx.x;
  int done = 0;
  for (int c0 = 0; c0 < a.n; c0 += 1024) {  // uniform trip count: every thread reaches the barriers
    const int i = c0 + tid;
    int code = -1;
    float x = 0.f, y = 0.f, vid = 0.f;
    float col[8], wgt[8], g[4];
    if (i < a.n) {
      vid = hs::init_videpth(a.tri[i] != 0, a.good[i] != 0, a.idepth[i], a.invz[i]);
      x = a.u[i] + 0.5f;
      y = a.v[i] + 0.5f;
      // the constructor runs only where its taps stay inside the image
      code = hs::init_rule(vid, true, x, y, a.W, a.H);
      if (code == hs::HS_INIT_SEEDED) {
        const bool fin = hs_imm::ctor_point(a.img, x, y, a.W, a.H, a.outlierTHSumComponent, col, wgt, g);
        code = hs::init_rule(vid, fin, x, y, a.W, a.H);
      }
      a.why[i] = (uint8_t)code;
    }
    int total;
    const int r = hs_imm::block_rank(code == hs::HS_INIT_SEEDED, wsum, &total);
    if (code == hs::HS_INIT_SEEDED && done + r < a.room) {
      // the new MapPoint (Src/System.cpp:277-286): idepth = idepth_zero = videpth, hasDepthPrior, no residual yet
      HsStagedPoint& s = a.out[a.base + done + r];
      s.u = x;
      s.v = y;
      s.idepth = vid;
      s.idepth_zero = vid;
      s.priorF = a.priorF;
      s.relBL = 0.f;
      s.nGood = 0;
#pragma unroll
      for (int q = 0; q < 8; q++) {
        s.color[q] = col[q];
        s.weight[q] = wgt[q];
      }
    }
    done += total;
  }
  if (tid == 0) *a.n_seeded = done;
}
