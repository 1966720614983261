// hs_fast_kernels.hip — the UseFAST branch of FeatureDetector::ExtractFeatures (include/hs_extract.h, "The FAST
// branch, as arithmetic"): cv::FAST 9-16 with non-maximum suppression, the sort by response, Ssc and its final pass.
//   hs_k_fast_resp   the response plane: a 64x16 tile (+3 px halo) through LDS, the 16 ring differences in registers,
//                    the best of the 16 arcs of 9 by a branch-free min / max ladder; u8, 0 where there is no corner
//   hs_k_fast_count  strict 3x3 maxima per row (a wave per row, ballot + popcount)
//   hs_k_fast_write  the maxima in raster order, by the row-count scheme of hs_k_ext_write
//   hs_k_fast_sort   one stable counting pass on the 8-bit response, descending: a block histogram, a scan, then one
//                    wave scatters 64 corners at a time with each lane's rank among the equal keys below it
//   hs_k_fast_ssc    a workgroup (one wave) per candidate width: the search bracket in fp64 from the corner count, a
//                    width outside it returns, the others are evaluated 64 corners at a time against their own
//                    byte-per-cell covered grid in global memory and leave their count and their taken corners
//   hs_k_fast_final  one wave: the reference's binary search over those counts names the width taken; then the border
//                    rule and the min_dist rule over its taken corners, 64 at a time against an occupancy image;
//                    writes x / y / response and the count where hs_k_ext_desc reads them
// The two greedy passes are exact a wave at a time: a lane survives if nothing taken before its batch covers it, the
// lowest survivor is what the sequential pass would take next, and it knocks out the survivors it covers.
#include "hs_extract_kernels.h"
#include "hs_fast_kernels.h"

namespace {

constexpr int R = kFastRing;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// strict 3x3 maximum of the response plane at (x, y), 1 <= x < W-1, 1 <= y < H-1
__device__ __forceinline__ bool is_max(const uint8_t* resp, int W, int x, int y, int* r_out) {
  const uint8_t* p = resp + (size_t)y * W + x;
  const int r = p[0];
  *r_out = r;
  const int m = max(max(max(p[-W - 1], p[-W]), max(p[-W + 1], p[-1])), max(max(p[1], p[W - 1]), max(p[W], p[W + 1])));
  return r > m;
}

}  // namespace

__global__ __launch_bounds__(256) void hs_k_fast_resp(HsFastArgs a) {
  constexpr int TW = kFastTileW, TH = kFastTileH;
  constexpr int SW = TW + 2 * R, SH = TH + 2 * R, SP = TW + 8;
  __shared__ uint8_t s_src[SH * SP];
  const int t = threadIdx.x;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  // texels outside the image are 0: only pixels within 3 px of an edge would read them, and their response is 0
  for (int i = t; i < SH * SW; i += 256) {
    const int r = i / SW, c = i - r * SW;
    const int gx = x0 + c - R, gy = y0 + r - R;
    uint8_t v = 0;
    if (gx >= 0 && gy >= 0 && gx < a.W && gy < a.H) v = a.img[(size_t)gy * a.W + gx];
    s_src[r * SP + c] = v;
  }
  __syncthreads();
  constexpr int dx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
  constexpr int dy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
  const int c = t & 63;
  const int x = x0 + c;
  if (x >= a.W) return;
#pragma unroll
  for (int j = 0; j < TH / 4; j++) {
    const int r = (t >> 6) + 4 * j;
    const int y = y0 + r;
    if (y >= a.H) break;
    int out = 0;
    if (x >= R && y >= R && x < a.W - R && y < a.H - R) {
      const uint8_t* p = s_src + (r + R) * SP + c + R;
      const int v = p[0];
      int d[16];
#pragma unroll
      for (int k = 0; k < 16; k++) d[k] = v - p[dy[k] * SP + dx[k]];
      // lo9[k] = min of d[k .. k+8], hi9[k] = max of the same (indices mod 16), by doubling
      int lo[16], hi[16], l2[16], h2[16];
#pragma unroll
      for (int k = 0; k < 16; k++) { lo[k] = min(d[k], d[(k + 1) & 15]); hi[k] = max(d[k], d[(k + 1) & 15]); }
#pragma unroll
      for (int k = 0; k < 16; k++) { l2[k] = min(lo[k], lo[(k + 2) & 15]); h2[k] = max(hi[k], hi[(k + 2) & 15]); }
#pragma unroll
      for (int k = 0; k < 16; k++) { lo[k] = min(l2[k], l2[(k + 4) & 15]); hi[k] = max(h2[k], h2[(k + 4) & 15]); }
      int dark = -256, bright = 256;  // max_k min(arc), min_k max(arc)
#pragma unroll
      for (int k = 0; k < 16; k++) {
        dark = max(dark, min(lo[k], d[(k + 8) & 15]));
        bright = min(bright, max(hi[k], d[(k + 8) & 15]));
      }
      const int s = max(dark, -bright);
      out = s > a.threshold ? s - 1 : 0;
    }
    a.resp[(size_t)y * a.W + x] = (uint8_t)out;
  }
}

__global__ __launch_bounds__(256) void hs_k_fast_count(HsFastArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);  // image row `row + 3`
  if (row >= a.H - 2 * R) return;
  const int x1 = a.W - R;
  int c = 0;
  for (int xb = R; xb < x1; xb += 64) {
    const int x = xb + lane;
    int r;
    const bool k = x < x1 && is_max(a.resp, a.W, x, row + R, &r);
    c += __popcll(__ballot(k));
  }
  if (lane == 0) a.row_cnt[row] = c;
}

__global__ __launch_bounds__(256) void hs_k_fast_write(HsFastArgs a) {
  const int lane = threadIdx.x & 63;
  const int rows = a.H - 2 * R;
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
  if (row == 0 && lane == 0) a.info[kFastInfoCorners] = total;
  const int x1 = a.W - R;
  for (int xb = R; xb < x1; xb += 64) {
    const int x = xb + lane;
    int r = 0;
    const bool k = x < x1 && is_max(a.resp, a.W, x, row + R, &r);
    const unsigned long long mask = __ballot(k);
    if (k) {
      const int pos = before + __popcll(mask & ((1ull << lane) - 1ull));
      a.c_idx[pos] = (row + R) * a.W + x;
      a.c_resp[pos] = (uint8_t)r;
    }
    before += __popcll(mask);
  }
}

__global__ __launch_bounds__(256) void hs_k_fast_sort(HsFastArgs a) {
  __shared__ int s_hist[256];
  __shared__ int s_cur[256];
  const int t = threadIdx.x;
  const int n = a.info[kFastInfoCorners];
  s_hist[t] = 0;
  __syncthreads();
  for (int i = t; i < n; i += 256) atomicAdd(&s_hist[a.c_resp[i]], 1);
  __syncthreads();
  int base = 0;  // corners with a larger response come first
  for (int k = 255; k > t; k--) base += s_hist[k];
  s_cur[t] = base;
  __syncthreads();
  if (t >= 64) return;
  const int lane = t;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int b0 = 0; b0 < n; b0 += 64) {
    const int i = b0 + lane;
    const bool valid = i < n;
    const int key = valid ? a.c_resp[i] : 0;
    unsigned long long same = __ballot(valid);  // the valid lanes of this batch with this lane's key
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (key >> b) & 1;
      const unsigned long long m = __ballot(bit);
      same &= bit ? m : ~m;
    }
    const int rank = __popcll(same & below), cnt = __popcll(same);
    const int pos = valid ? s_cur[key] + rank : 0;
    if (valid) {
      a.s_idx[pos] = a.c_idx[i];
      a.s_resp[pos] = (uint8_t)key;
    }
    __builtin_amdgcn_wave_barrier();  // every lane of a group has read the bin before its last lane advances it
    if (valid && rank == cnt - 1) s_cur[key] += cnt;
    __builtin_amdgcn_wave_barrier();  // and the next batch reads it after that
  }
}

namespace {

// Ssc's search bracket for n >= 2 corners (Src/Detector.cpp:457-474), as include/hs_extract.h words it
struct Bracket {
  int low, high;
  unsigned Kmin, Kmax;
};

__device__ __forceinline__ Bracket ssc_bracket(const HsFastArgs& a, int n) {
  const int W = a.W, H = a.H;
  const int K = min(a.num_features, n);
  const int exp1 = H + W + 2 * K;
  const long long exp2 = 4LL * W + 4LL * K + 4LL * H * K + (long long)H * H + (long long)W * W - 2LL * H * W +
                         4LL * H * W * K;
  const double exp3 = sqrt((double)exp2);
  const double exp4 = K - 1;
  const double sol1 = -round((exp1 + exp3) / exp4);
  const double sol2 = -round((exp1 - exp3) / exp4);
  Bracket b;
  b.high = (int)(sol1 > sol2 ? sol1 : sol2);
  b.low = (int)floor(sqrt((double)(n / K)));
  const float Kf = (float)K;
  const float kt = Kf * a.tolerance;
  b.Kmin = (unsigned)roundf(Kf - kt);
  b.Kmax = (unsigned)roundf(Kf + kt);
  return b;
}

}  // namespace

// One workgroup (one wave) per candidate width w = blockIdx.x + 1: the widths of a search are independent of each
// other once the sorted corner list exists.  A width outside [low, high] returns at once.  Each width has its own
// covered grid and its own list of taken corners (offsets from the host's tables), and leaves its count in wcnt.
__global__ __launch_bounds__(64) void hs_k_fast_ssc(HsFastArgs a) {
  const int lane = threadIdx.x;
  const int n = a.info[kFastInfoCorners];
  const int W = a.W, H = a.H;
  if (n <= 1) return;  // no search (hs_k_fast_final)
  const Bracket br = ssc_bracket(a, n);
  const int w = blockIdx.x + 1;
  if (w < br.low || w > br.high) return;
  uint8_t* covered = a.covered + a.woff[w - 1];
  int* taken = a.wtaken + a.toff[w - 1];
  const int mr = lane / 5 - 2, mc = lane % 5 - 2;  // this lane's cell of a taken corner's 5x5 (lanes 0..24)
  int cnt = 0;
  {
    const int nrows = 2 * H / w, ncols = 2 * W / w;
    const size_t pitch = (size_t)ncols + 1;
    const size_t cells = (size_t)(nrows + 1) * pitch;
    uint4* cov16 = reinterpret_cast<uint4*>(covered);  // every grid starts 16-byte aligned and is padded to 16
    for (size_t i = lane; i < (cells + 15) / 16; i += 64) cov16[i] = make_uint4(0, 0, 0, 0);
    __threadfence();
    for (int b0 = 0; b0 < n; b0 += 64) {
      const int i = b0 + lane;
      const bool valid = i < n;
      const int p = valid ? a.s_idx[i] : 0;
      const int y = p / W, x = p - y * W;
      const int cr = 2 * y / w, cc = 2 * x / w;
      bool surv = valid && covered[cr * pitch + cc] == 0;
      while (true) {
        const unsigned long long m = __ballot(surv);
        if (!m) break;
        const int l = __ffsll((long long)m) - 1;
        const int tr = __builtin_amdgcn_readlane(cr, l), tc = __builtin_amdgcn_readlane(cc, l);
        if (lane == l) {
          taken[cnt] = i;
          surv = false;
        }
        cnt++;
        if (lane < 25) {
          const int r = tr + mr, c = tc + mc;
          if (r >= 0 && r <= nrows && c >= 0 && c <= ncols) covered[r * pitch + c] = 1;
        }
        if (surv && abs(cr - tr) <= 2 && abs(cc - tc) <= 2) surv = false;
      }
      // this batch's marks, written by other lanes, before the next batch's reads: the fence orders the memory,
      // the barrier the lanes
      __threadfence();
      __builtin_amdgcn_wave_barrier();
    }
  }
  if (lane == 0) a.wcnt[w - 1] = cnt;
}

// One wave: the reference's binary search over the counts hs_k_fast_ssc stored names the width taken; then the
// final pass over that width's taken corners.
__global__ __launch_bounds__(64) void hs_k_fast_final(HsFastArgs a) {
  const int lane = threadIdx.x;
  const int n = a.info[kFastInfoCorners];
  const int W = a.W, H = a.H, d = a.min_dist;  // min_dist clipped to the image's larger side by the host
  int nt = n, taken_w = -1, b_low = 1, b_high = 0;  // n <= 1: no search, the corner (if any) is the result
  if (n > 1) {
    const Bracket br = ssc_bracket(a, n);
    int low = br.low, high = br.high, prev = -1;
    b_low = low;
    b_high = high;
    nt = 0;
    while (true) {
      const int w = low + (high - low) / 2;
      if (w == prev || low > high) break;
      if (w > a.max_high) {  // a width no workgroup evaluated: the grid's bound would be wrong
        taken_w = -2;
        nt = 0;
        break;
      }
      const int cnt = a.wcnt[w - 1];
      taken_w = w;
      nt = cnt;
      if ((unsigned)cnt >= br.Kmin && (unsigned)cnt <= br.Kmax) break;
      if ((unsigned)cnt < br.Kmin) high = w - 1;
      else low = w + 1;
      prev = w;
    }
  }
  if (lane == 0) {
    a.info[kFastInfoWidth] = taken_w;
    a.info[kFastInfoTaken] = nt;
    a.info[kFastInfoLow] = b_low;
    a.info[kFastInfoHigh] = b_high;
  }
  const int* taken = a.wtaken + (taken_w > 0 ? a.toff[taken_w - 1] : 0);
  int kept = 0;
  for (int b0 = 0; b0 < nt; b0 += 64) {
    const int i = b0 + lane;
    const bool valid = i < nt;
    const int j = valid && n > 1 ? taken[i] : 0;
    const int p = valid ? a.s_idx[j] : 0;
    const int r = valid ? a.s_resp[j] : 0;
    const int y = p / W, x = p - y * W;
    bool surv = valid && !(x < kExtBorder || x > W - kExtBorder || y < kExtBorder || y > H - kExtBorder) && a.occ[p] == 0;
    while (true) {
      const unsigned long long m = __ballot(surv);
      if (!m) break;
      const int l = __ffsll((long long)m) - 1;
      const int tx = __builtin_amdgcn_readlane(x, l), ty = __builtin_amdgcn_readlane(y, l);
      if (lane == l) {
        if (kept < a.cap) {
          a.x[kept] = (float)x;
          a.y[kept] = (float)y;
          a.response[kept] = (float)r;
        }
        surv = false;
      }
      kept++;
      // the (2d+1)^2 square clipped to the image, a lane per column
      const int xa = max(tx - d, 0), xb = min(tx + d, W - 1), ya = max(ty - d, 0), yb = min(ty + d, H - 1);
      for (int xx = xa + lane; xx <= xb; xx += 64)
        for (int yy = ya; yy <= yb; yy++) a.occ[(size_t)yy * W + xx] = 1;
      if (surv && abs(x - tx) <= d && abs(y - ty) <= d) surv = false;
    }
    __threadfence();
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) *a.count = kept;
}
