// hs_image_kernels.hip — Frame::CreateDirPyrs (Src/Frame.cpp:104-181) on the device: every level of a frame's
// direct-image pyramid (I, dI/dx, dI/dy), absSquaredGrad and cvImgL in two launches.  The library's one pyramid
// implementation: hs_img_build (hs_image.cpp) launches it for the device image and for every context's own frame.
//   hs_k_img_levels  one workgroup per 32 x 32 tile of level 0.  A thread forms the level-0 intensity of 4 of the
//                    tile's pixels -- a plain load of the float frame (ImageData::fImgL), or the undistorted pixel of
//                    a raw u8 frame (hs_undist_px.h, the arithmetic of hs_k_undistort, with its img8) -- writes the
//                    texel (I, 0, 0, 0) and cvImgL and keeps I in LDS; with neither source it reads I from the level-0
//                    texel already in place and leaves that level alone.  The workgroup then folds the tile into
//                    levels 1..L-1 in LDS, 0.25f * (((tl + tr) + bl) + br) in the reference's operation order,
//                    writing each level's texels as it goes.  A pixel exists at level l iff x < W >> l and y < H >> l
//                    (CalibData's wpyr / hpyr rule); its four sources then exist at level l-1 and, the tile's side
//                    being a multiple of 2^(L-1), lie in the same tile.  Pixels that do not exist (partial tiles at
//                    the right and bottom, the odd last column / row of a level) are computed from whatever their
//                    sources hold and never stored.
//   hs_k_img_grads   central differences over the interior index range [w, w*(h-1)) of each level (row-wrapped at the
//                    left / right columns exactly as the reference's linear index loop), non-finite -> 0, and
//                    absSquaredGrad = dx*dx + dy*dy (the gamma weighting is skipped: Calib->PhotoUnDistL is null,
//                    SURVEY.md Appendix B quirk 4).  The first and last rows keep dI = 0 (the reference leaves them
//                    uninitialised).  All levels in one grid (a workgroup belongs to one level); a level the launcher
//                    gives no blocks (those below its first level) is never selected.  A separate launch: it reads
//                    the neighbours' intensities, which other workgroups of hs_k_img_levels wrote.
// Latency-bound, not bandwidth-bound (a 640 x 480 frame moves ~7 MB): what the fusion saves is launches.
#include "hs_image_kernels.h"
#include "hs_undist_px.h"

#pragma clang fp contract(off)

namespace {
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
  if (a.raw) {
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
      if (a.fimg || a.raw) {
        f = a.fimg ? a.fimg[i]
                   : undistort_px(a.raw, sBinv, a.Binv != nullptr, a.vinv, a.map, a.w_in, a.h_in, a.passthrough, i);
        a.lvl[0][i] = make_float4(f, 0.f, 0.f, 0.f);
        if (a.img8) a.img8[i] = (uint8_t)(a.B ? sat8(sB[sat8(f)]) : sat8(f));
      } else {
        f = a.lvl[0][i].x;  // level 0 in place: its gradient lanes are the owner's
      }
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
  if (absg) absg[i] = g;
}
