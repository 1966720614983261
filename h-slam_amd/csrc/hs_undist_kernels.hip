// hs_undist_kernels.hip — DatasetReader::undistort fused into one gather kernel: the photometric correction is
// applied to each of the four taps as it is read (the same float the reference's first pass would have stored),
// then cv::remap's INTER_LINEAR arithmetic (include/hs_undist.h) in float, left to right, unfused (hs_undist_px.h).
// One output pixel per thread; memory-bound (8 B of map, 4 cached byte taps, 4 B out per pixel).
#include "hs_undist_kernels.h"
#include "hs_undist_px.h"

__global__ __launch_bounds__(256) void hs_k_undistort(HsUndistArgs a) {
  __shared__ float sBinv[256];
  __shared__ float sB[256];
  const int t = threadIdx.x;
  if (a.Binv) sBinv[t] = a.Binv[t];
  if (a.B) sB[t] = a.B[t];
  __syncthreads();
  const int i = blockIdx.x * 256 + t;
  if (i >= a.n_out) return;
  const float f = undistort_px(a.raw, sBinv, a.Binv != nullptr, a.vinv, a.map, a.w_in, a.h_in, a.passthrough, i);
  if (a.fimg) a.fimg[i] = f;
  if (a.img8) a.img8[i] = (uint8_t)(a.B ? sat8(sB[sat8(f)]) : sat8(f));
}
