// hs_extract_kernels.hip — FeatureDetector::ExtractFeatures' per-keyframe image work (include/hs_extract.h):
//   hs_k_ext_blur   the 7x7 fixed-point Gaussian, separable, one 64x16 tile (+3 px halo) per block through LDS
//   hs_k_ext_count  keys per interior row of the selection map (a wave per row, ballot + popcount)
//   hs_k_ext_write  the keys in raster order: a row's offset is the sum of the rows before it, a key's place in its
//                   row the popcount of the ballot below its lane; no atomics, the order is fixed by the map alone
//   hs_k_ext_desc   a wave per key: IC_Angle's moments reduced across the lanes, fastAtan2, then 4 of the 256
//                   comparisons per lane, gathered into the descriptor by 4 ballots and stored as 8 dwords
// Every gather is in bounds by the rules of include/hs_extract.h (keys >= 19 px from the edges, taps <= 18 px).
#include "hs_extract_kernels.h"

namespace {

constexpr int B = kExtBorder;

// BORDER_REFLECT_101 for i in [-3, n + 2], n >= 4
__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// cv::fastAtan2's scalar form in float (degrees); every operation rounded, none fused (-ffp-contract=off)
__device__ __forceinline__ float fast_atan2_deg(float y, float x) {
  const float scale = (float)(180.0 / 3.14159265358979323846);
  const float p1 = 0.9997878412794807f * scale, p3 = -0.3258083974640975f * scale;
  const float p5 = 0.1555786518463281f * scale, p7 = -0.04432655554792128f * scale;
  const float eps = 2.220446049250313e-16f;  // (float)DBL_EPSILON
  const float ax = fabsf(x), ay = fabsf(y);
  float a, c, c2;
  if (ax >= ay) {
    c = ay / (ax + eps);
    c2 = c * c;
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  } else {
    c = ax / (ay + eps);
    c2 = c * c;
    a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  }
  if (x < 0) a = 180.f - a;
  if (y < 0) a = 360.f - a;
  return a;
}

}  // namespace

__global__ __launch_bounds__(256) void hs_k_ext_blur(HsExtBlurArgs a) {
  constexpr int TW = kExtBlurTileW, TH = kExtBlurTileH;
  constexpr int SW = TW + 6, SH = TH + 6, SP = TW + 8;  // source tile with its halo; row pitch in bytes
  __shared__ uint8_t s_src[SH * SP];
  __shared__ uint16_t s_h[SH * TW];
  const int t = threadIdx.x;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int w0 = a.w[0], w1 = a.w[1], w2 = a.w[2], w3 = a.w[3];

  // source tile, the border rule applied here; texels that no pixel of the image needs (a partial tile) are 0
  for (int i = t; i < SH * SW; i += 256) {
    const int r = i / SW, c = i - r * SW;
    const int gx = x0 + c - 3, gy = y0 + r - 3;
    uint8_t v = 0;
    if (gx < a.W + 3 && gy < a.H + 3) v = a.src[(size_t)reflect101(gy, a.H) * a.W + reflect101(gx, a.W)];
    s_src[r * SP + c] = v;
  }
  __syncthreads();

  // rows: SH rows x 16 groups of 4 pixels
  for (int i = t; i < SH * (TW / 4); i += 256) {
    const int r = i >> 4, q = (i & 15) * 4;
    int v[10];
#pragma unroll
    for (int k = 0; k < 10; k++) v[k] = s_src[r * SP + q + k];
#pragma unroll
    for (int j = 0; j < 4; j++)
      s_h[r * TW + q + j] =
          (uint16_t)(w0 * (v[j] + v[j + 6]) + w1 * (v[j + 1] + v[j + 5]) + w2 * (v[j + 2] + v[j + 4]) + w3 * v[j + 3]);
  }
  __syncthreads();

  // columns: 4 pixels of one row per thread
  const int r = t >> 4, q = (t & 15) * 4;
  const int x = x0 + q, y = y0 + r;
  if (y >= a.H || x >= a.W) return;
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint16_t* h = s_h + r * TW + q + j;
    const uint32_t v = (uint32_t)w0 * (h[0] + h[6 * TW]) + (uint32_t)w1 * (h[TW] + h[5 * TW]) +
                       (uint32_t)w2 * (h[2 * TW] + h[4 * TW]) + (uint32_t)w3 * h[3 * TW];
    o[j] = (v + 32768u) >> 16;
  }
  uint8_t* d = a.dst + (size_t)y * a.W + x;
  if ((a.W & 3) == 0) {  // x is a multiple of 4, so is y * W: a whole aligned dword lies inside the row
    *reinterpret_cast<uint32_t*>(d) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (x + j < a.W) d[j] = (uint8_t)o[j];
  }
}

__global__ __launch_bounds__(256) void hs_k_ext_count(HsExtKeysArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);  // interior row: image row `row + B`
  if (row >= a.H - 2 * B) return;
  const float* m = a.map + (size_t)(row + B) * a.W;
  const int x1 = a.W - B;
  int c = 0;
  for (int xb = B; xb < x1; xb += 64) {
    const int x = xb + lane;
    const bool k = x < x1 && m[x] != 0.f;
    c += __popcll(__ballot(k));
  }
  if (lane == 0) a.row_cnt[row] = c;
}

__global__ __launch_bounds__(256) void hs_k_ext_write(HsExtKeysArgs a) {
  const int lane = threadIdx.x & 63;
  const int rows = a.H - 2 * B;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  int before = 0, total = 0;
  for (int r = lane; r < rows; r += 64) {
    const int c = a.row_cnt[r];
    total += c;
    if (r < row) before += c;
  }
  before = wave_sum(before);
  total = wave_sum(total);
  if (row == 0 && lane == 0) *a.count = total;
  if (total > a.cap) return;  // the host reports the overflow; nothing is written
  const float* m = a.map + (size_t)(row + B) * a.W;
  const int x1 = a.W - B;
  for (int xb = B; xb < x1; xb += 64) {
    const int x = xb + lane;
    const bool k = x < x1 && m[x] != 0.f;
    const unsigned long long mask = __ballot(k);
    if (k) {
      const int pos = before + __popcll(mask & ((1ull << lane) - 1ull));
      a.x[pos] = (float)x;
      a.y[pos] = (float)(row + B);
    }
    before += __popcll(mask);
  }
}

__global__ __launch_bounds__(256) void hs_k_ext_desc(HsExtDescArgs a) {
  const int lane = threadIdx.x & 63;
  const int n = *a.count;
  if (n > a.cap) return;
  const int nwaves = gridDim.x * 4;
  const int W = a.W;
  const unsigned long long umax = a.umax;
  char4 pat[4];
#pragma unroll
  for (int j = 0; j < 4; j++) pat[j] = a.pattern[j * 64 + lane];
  const int u = (lane & 31) - kExtHalfPatch;  // the disc's column of this lane (lane 31 of each half has none)

  for (int key = blockIdx.x * 4 + (threadIdx.x >> 6); key < n; key += nwaves) {
    const int x = (int)a.x[key], y = (int)a.y[key];
    const size_t centre = (size_t)y * W + x;
    const uint8_t* c = a.img + centre;
    int m10 = 0, m01 = 0;
    for (int r = lane >> 5; r <= 2 * kExtHalfPatch; r += 2) {  // the two half-waves take alternate rows
      const int v = r - kExtHalfPatch;
      const int d = (int)((umax >> (4 * (v < 0 ? -v : v))) & 15);
      if (u >= -d && u <= d) {
        const int I = c[v * W + u];
        m10 += u * I;
        m01 += v * I;
      }
    }
    m10 = wave_sum(m10);
    m01 = wave_sum(m01);
    const float ang = fast_atan2_deg((float)m01, (float)m10);
    const float rad = ang * (float)(3.14159265358979323846 / 180.0);
    const float ca = (float)cos((double)rad), sb = (float)sin((double)rad);
    const uint8_t* bc = a.blurred + centre;
    auto val = [&](int px, int py) -> int {
      const float fx = (float)px, fy = (float)py;
      const int yo = __float2int_rn(fx * sb + fy * ca);
      const int xo = __float2int_rn(fx * ca - fy * sb);
      return bc[yo * W + xo];
    };
    unsigned long long bits[4];
#pragma unroll
    for (int j = 0; j < 4; j++) bits[j] = __ballot(val(pat[j].x, pat[j].y) < val(pat[j].z, pat[j].w));
    if (lane == 0) a.angle[key] = ang;
    if (lane < 8) {
      const unsigned long long mm = (lane >> 1) == 0 ? bits[0] : ((lane >> 1) == 1 ? bits[1] : ((lane >> 1) == 2 ? bits[2] : bits[3]));
      a.desc[(size_t)key * 8 + lane] = (uint32_t)(mm >> (32 * (lane & 1)));
    }
  }
}
