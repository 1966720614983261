// hs_image_kernels.hip — one camera frame into every level of its direct-image pyramid in two launches
// (include/hs_image.h), in place of the 2L+1 of hs_undist_enqueue + hs_build_dir_pyramid, and bit-identical to them:
//   hs_k_img_levels  one workgroup per 32 x 32 tile of level 0.  A thread forms the level-0 intensity of 4 of the
//                    tile's pixels -- hs_k_undistort's arithmetic (include/hs_undist.h: the same taps, weights and
//                    unfused left-to-right sum, the same img8) or a plain load of the float frame -- writes the texel
//                    (I, 0, 0, 0) and cvImgL and keeps I in LDS; the workgroup then folds the tile into levels
//                    1..L-1 in LDS, 0.25f * (((tl + tr) + bl) + br) as hs_k_pyr_down, writing each level's texels as
//                    it goes.  A pixel exists at level l iff x < W >> l and y < H >> l; its four sources then exist at
//                    level l-1 and, the tile's side being a multiple of 2^(L-1), lie in the same tile.  Pixels that do
//                    not exist (partial tiles at the right and bottom, the odd last column / row of a level) are
//                    computed from whatever their sources hold and never stored.
//   hs_k_img_grads   hs_k_pyr_grad's arithmetic over the texels of all levels in one grid (a workgroup belongs to
//                    one level).  A separate launch: it reads the neighbours' intensities, which other workgroups of
//                    hs_k_img_levels wrote.
// Latency-bound, not bandwidth-bound (a 640 x 480 frame moves ~7 MB): what the fusion saves is launches.
#include "hs_image_kernels.h"

#pragma clang fp contract(off)

namespace {
// cv::saturate_cast<uchar>(float): round half to even, clamped to 0..255
__device__ __forceinline__ int sat8(float v) {
  const int r = __float2int_rn(v);
  return r < 0 ? 0 : (r > 255 ? 255 : r);
}

// hs_k_undistort's value of output pixel i
__device__ __forceinline__ float undistort_px(const HsImgLevelsArgs& a, const float* sBinv, int i) {
  auto tap = [&](int j) -> float {
    const int p = a.raw[j];
    float v = a.Binv ? sBinv[p] : (float)p;
    if (a.vinv) v = v * a.vinv[j];
    return v;
  };
  if (a.passthrough) return tap(i);
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
  return s00 * w0 + s01 * w1 + s10 * w2 + s11 * w3;
}

// LDS offset of level l's (kImgTile >> l)^2 block: 0, 1024, 1280, 1344, 1360, 1364
constexpr int lds_off(int l) {
  int o = 0;
  for (int k = 0; k < l; k++) o += (kImgTile >> k) * (kImgTile >> k);
  return o;
}
}  // namespace

__global__ __launch_bounds__(kImgThreads) void hs_k_img_levels(HsImgLevelsArgs a) {
  __shared__ float sBinv[256];
  __shared__ float sB[256];
  __shared__ float sI[lds_off(HS_MAX_LEVELS)];
  static_assert(kImgThreads == 256 && kImgTile == 32, "a thread per table entry, 8 tile rows per pass");
  const int t = threadIdx.x;
  if (!a.fimg) {
    if (a.Binv) sBinv[t] = a.Binv[t];
    if (a.B) sB[t] = a.B[t];
    __syncthreads();
  }
  const int x0 = blockIdx.x * kImgTile, y0 = blockIdx.y * kImgTile;
  const int tx = t & (kImgTile - 1), ty = t >> 5;
  const int x = x0 + tx;
#pragma unroll
  for (int k = 0; k < kImgTile / 8; k++) {
    const int ly = ty + 8 * k, y = y0 + ly;
    float f = 0.f;
    if (x < a.W && y < a.H) {
      const int i = y * a.W + x;
      f = a.fimg ? a.fimg[i] : undistort_px(a, sBinv, i);
      a.lvl[0][i] = make_float4(f, 0.f, 0.f, 0.f);
      if (a.img8) a.img8[i] = (uint8_t)(a.B ? sat8(sB[sat8(f)]) : sat8(f));
    }
    sI[ly * kImgTile + tx] = f;
  }
  __syncthreads();
#pragma unroll
  for (int l = 1; l < HS_MAX_LEVELS; l++) {
    if (l >= a.nlev) break;  // the same in every thread
    const int side = kImgTile >> l;
    const float* src = sI + lds_off(l - 1);
    float* dst = sI + lds_off(l);
    if (t < side * side) {
      const int lx = t & (side - 1), ly = t >> (5 - l);
      const int b = 2 * lx + 2 * ly * (2 * side);
      const float v = 0.25f * (((src[b] + src[b + 1]) + src[b + 2 * side]) + src[b + 1 + 2 * side]);
      dst[t] = v;
      const int wl = a.W >> l, hl = a.H >> l;
      const int gx = (x0 >> l) + lx, gy = (y0 >> l) + ly;
      if (gx < wl && gy < hl) a.lvl[l][gy * wl + gx] = make_float4(v, 0.f, 0.f, 0.f);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void hs_k_img_grads(HsImgGradsArgs a) {
  // the workgroup's level, by selects on constants' indices: no array of the arguments is indexed at run time
  int b0 = 0, wl = a.w[0], hl = a.h[0];
  float4* lvl = a.lvl[0];
  float* absg = a.absg[0];
#pragma unroll
  for (int k = 1; k < HS_MAX_LEVELS; k++)
    if (k < a.nlev && (int)blockIdx.x >= a.boff[k]) {
      b0 = a.boff[k];
      wl = a.w[k];
      hl = a.h[k];
      lvl = a.lvl[k];
      absg = a.absg[k];
    }
  const int i = ((int)blockIdx.x - b0) * 256 + (int)threadIdx.x;
  if (i >= wl * hl) return;
  const float* s = reinterpret_cast<const float*>(lvl);
  float dx = 0.f, dy = 0.f, g = 0.f;
  const bool interior = i >= wl && i < wl * (hl - 1);
  if (interior) {
    dx = 0.5f * (s[4 * (i + 1)] - s[4 * (i - 1)]);
    dy = 0.5f * (s[4 * (i + wl)] - s[4 * (i - wl)]);
    if (!isfinite(dx)) dx = 0.f;
    if (!isfinite(dy)) dy = 0.f;
    g = dx * dx + dy * dy;
  }
  // threads read the neighbours' intensity lanes and write only their own gradient lanes (no overlap)
  reinterpret_cast<float*>(lvl + i)[1] = dx;
  reinterpret_cast<float*>(lvl + i)[2] = dy;
  absg[i] = g;
}
