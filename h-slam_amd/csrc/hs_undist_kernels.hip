// hs_undist_kernels.hip — DatasetReader::undistort fused into one gather kernel: the photometric correction is
// applied to each of the four taps as it is read (the same float the reference's first pass would have stored),
// then cv::remap's INTER_LINEAR arithmetic (include/hs_undist.h) in float, left to right, unfused.
// One output pixel per thread; memory-bound (8 B of map, 4 cached byte taps, 4 B out per pixel).
#include "hs_undist_kernels.h"

namespace {
// cv::saturate_cast<uchar>(float): round half to even, clamped to 0..255
__device__ __forceinline__ int sat8(float v) {
  const int r = __float2int_rn(v);
  return r < 0 ? 0 : (r > 255 ? 255 : r);
}
}  // namespace

__global__ __launch_bounds__(256) void hs_k_undistort(HsUndistArgs a) {
  __shared__ float sBinv[256];
  __shared__ float sB[256];
  const int t = threadIdx.x;
  if (a.Binv) sBinv[t] = a.Binv[t];
  if (a.B) sB[t] = a.B[t];
  __syncthreads();
  const int i = blockIdx.x * 256 + t;
  if (i >= a.n_out) return;

  // the tap value S(p) of source index j
  auto tap = [&](int j) -> float {
    const int p = a.raw[j];
    float v = a.Binv ? sBinv[p] : (float)p;
    if (a.vinv) v = v * a.vinv[j];
    return v;
  };

  float f;
  if (a.passthrough) {
    f = tap(i);
  } else {
    const int2 s = a.map[i];
    const int ix = s.x >> 5, iy = s.y >> 5;
    const float fx = (float)(s.x & 31) * (1.f / 32), fy = (float)(s.y & 31) * (1.f / 32);
    const float w0 = (1.f - fy) * (1.f - fx), w1 = (1.f - fy) * fx, w2 = fy * (1.f - fx), w3 = fy * fx;
    const bool x0 = ix >= 0 && ix < a.w_in, x1 = ix + 1 >= 0 && ix + 1 < a.w_in;
    const bool y0 = iy >= 0 && iy < a.h_in, y1 = iy + 1 >= 0 && iy + 1 < a.h_in;
    const int j = iy * a.w_in + ix;
    const float s00 = (x0 && y0) ? tap(j) : 0.f;
    const float s01 = (x1 && y0) ? tap(j + 1) : 0.f;
    const float s10 = (x0 && y1) ? tap(j + a.w_in) : 0.f;
    const float s11 = (x1 && y1) ? tap(j + a.w_in + 1) : 0.f;
    f = s00 * w0 + s01 * w1 + s10 * w2 + s11 * w3;
  }
  if (a.fimg) a.fimg[i] = f;
  if (a.img8) a.img8[i] = (uint8_t)(a.B ? sat8(sB[sat8(f)]) : sat8(f));
}
