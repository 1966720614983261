// hs_undist_px.h — one output pixel of DatasetReader::undistort (include/hs_undist.h), for the kernels that form it:
// hs_k_undistort (a float plane / cvImgL) and hs_k_img_levels (level 0 of a pyramid).  Device code; the including
// file keeps floating-point contraction off.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// cv::saturate_cast<uchar>(float): round half to even, clamped to 0..255
__device__ __forceinline__ int sat8(float v) {
  const int r = __float2int_rn(v);
  return r < 0 ? 0 : (r > 255 ? 255 : r);
}

// The value of output pixel i: the photometric correction applied to each of the four taps as it is read (sBinv: the
// workgroup's copy of Binv, read where `gamma`; vinv: null = no vignette), then cv::remap's INTER_LINEAR arithmetic
// in float, left to right, unfused.  passthrough: pixel i = S(raw[i]), the map is not read.
__device__ __forceinline__ float undistort_px(const uint8_t* raw, const float* sBinv, bool gamma, const float* vinv,
                                              const int2* map, int w_in, int h_in, int passthrough, int i) {
  // the tap value S(p) of source index j
  auto tap = [&](int j) -> float {
    const int p = raw[j];
    float v = gamma ? sBinv[p] : (float)p;
    if (vinv) v = v * vinv[j];
    return v;
  };
  if (passthrough) return tap(i);
  const int2 s = map[i];
  const int ix = s.x >> 5, iy = s.y >> 5;
  const float fx = (float)(s.x & 31) * (1.f / 32), fy = (float)(s.y & 31) * (1.f / 32);
  const float w0 = (1.f - fy) * (1.f - fx), w1 = (1.f - fy) * fx, w2 = fy * (1.f - fx), w3 = fy * fx;
  const bool x0 = ix >= 0 && ix < w_in, x1 = ix + 1 >= 0 && ix + 1 < w_in;
  const bool y0 = iy >= 0 && iy < h_in, y1 = iy + 1 >= 0 && iy + 1 < h_in;
  const int j = iy * w_in + ix;
  const float s00 = (x0 && y0) ? tap(j) : 0.f;
  const float s01 = (x1 && y0) ? tap(j + 1) : 0.f;
  const float s10 = (x0 && y1) ? tap(j + w_in) : 0.f;
  const float s11 = (x1 && y1) ? tap(j + w_in + 1) : 0.f;
  return s00 * w0 + s01 * w1 + s10 * w2 + s11 * w3;
}
