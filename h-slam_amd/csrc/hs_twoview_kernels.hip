// hs_twoview_kernels.hip — the two-view fit of include/hs_twoview.h (the contract is stated there; tests/twoview_ref.py
// restates it in numpy).  Every sum that decides something is an integer sum or an fp64 sum in a fixed order, so a fit
// is bit-reproducible run to run.
#include "hs_twoview_kernels.h"

#include "hs_jacobi.h"
#include "hs_twoview_rule.h"

namespace {

constexpr int kBlock = 256;

// sum256 of the header: the caller's strided partial, then the fixed halving tree
__device__ double block_sum(double v, double* sh) {
  const int t = threadIdx.x;
  __syncthreads();  // sh may still be read from the sum before
  sh[t] = v;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (t < s) sh[t] = sh[t] + sh[t + s];
    __syncthreads();
  }
  return sh[0];
}

__device__ inline unsigned ordered_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ inline float from_ordered_key(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the k-th smallest (0-based) of v[i * stride] over the i with f[i] != 0, exactly: four passes of an 8-bit radix
// histogram over the ordered bit pattern (integer counts only).  k must be below the number of flagged values.
__device__ float block_select(const float* v, int stride, const uint8_t* f, int n, int k, unsigned* hist,
                              unsigned* ctl) {
  const int t = threadIdx.x;
  unsigned prefix = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    __syncthreads();
    hist[t] = 0;
    if (t == 0) {
      ctl[0] = 0;
      ctl[1] = 0;
    }
    __syncthreads();
    for (int i = t; i < n; i += kBlock) {
      if (!f[i]) continue;
      const unsigned key = ordered_key(v[(size_t)i * stride]);
      if (shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (t == 0) {
      unsigned acc = 0;
      for (int d = 0; d < 256; d++) {
        if ((unsigned)k < acc + hist[d]) {
          ctl[0] = (unsigned)d;
          ctl[1] = (unsigned)k - acc;
          break;
        }
        acc += hist[d];
      }
    }
    __syncthreads();
    prefix |= ctl[0] << shift;
    k = (int)ctl[1];
  }
  return from_ordered_key(prefix);
}

// CheckHomography's body for one match (:677-720): the two score contributions (0 where none is added) and bIn
__device__ inline bool score_h(const float* H, const float* Hi, float4 k, float* c1, float* c2) {
  const float th = 5.991f;
  const float u1 = k.x, v1 = k.y, u2 = k.z, v2 = k.w;
  bool in = true;
  const float w2 = (float)(1.0 / (double)((Hi[6] * u2 + Hi[7] * v2) + Hi[8]));
  const float u2in1 = ((Hi[0] * u2 + Hi[1] * v2) + Hi[2]) * w2;
  const float v2in1 = ((Hi[3] * u2 + Hi[4] * v2) + Hi[5]) * w2;
  const float chi1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
  *c1 = 0.f;
  if (chi1 > th) in = false;
  else *c1 = th - chi1;
  const float w1 = (float)(1.0 / (double)((H[6] * u1 + H[7] * v1) + H[8]));
  const float u1in2 = ((H[0] * u1 + H[1] * v1) + H[2]) * w1;
  const float v1in2 = ((H[3] * u1 + H[4] * v1) + H[5]) * w1;
  const float chi2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
  *c2 = 0.f;
  if (chi2 > th) in = false;
  else *c2 = th - chi2;
  return in;
}

// CheckFundamental's body for one match (:758-805)
__device__ inline bool score_f(const float* F, float4 k, float* c1, float* c2) {
  const float th = 3.841f, thScore = 5.991f;
  const float u1 = k.x, v1 = k.y, u2 = k.z, v2 = k.w;
  bool in = true;
  const float a2 = (F[0] * u1 + F[1] * v1) + F[2];
  const float b2 = (F[3] * u1 + F[4] * v1) + F[5];
  const float c2_ = (F[6] * u1 + F[7] * v1) + F[8];
  const float num2 = (a2 * u2 + b2 * v2) + c2_;
  const float chi1 = num2 * num2 / (a2 * a2 + b2 * b2);
  *c1 = 0.f;
  if (chi1 > th) in = false;
  else *c1 = thScore - chi1;
  const float a1 = (F[0] * u2 + F[3] * v2) + F[6];
  const float b1 = (F[1] * u2 + F[4] * v2) + F[7];
  const float c1_ = (F[2] * u2 + F[5] * v2) + F[8];
  const float num1 = (a1 * u1 + b1 * v1) + c1_;
  const float chi2 = num1 * num1 / (a1 * a1 + b1 * b1);
  *c2 = 0.f;
  if (chi2 > th) in = false;
  else *c2 = thScore - chi2;
  return in;
}

// the lowest index that attains the maximum of the scores above 0 (a NaN never wins: the reference's strict >);
// -1 when there is none.  sv / si: 256 entries each.
__device__ int block_argmax(const float* scores, int ns, float* sv, int* si, float* best_score) {
  const int t = threadIdx.x;
  __syncthreads();
  float v = t < ns ? scores[t] : 0.f;
  if (!(v > 0.f)) v = 0.f;
  sv[t] = v;
  si[t] = t;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (t < s) {
      const float ov = sv[t + s];
      const int oi = si[t + s];
      if (ov > sv[t] || (ov == sv[t] && oi < si[t])) {
        sv[t] = ov;
        si[t] = oi;
      }
    }
    __syncthreads();
  }
  *best_score = sv[0];
  return sv[0] > 0.f ? si[0] : -1;
}

__device__ inline void store_rt(float* dst, const double* R, const double* t, double sign_t) {
  for (int i = 0; i < 9; i++) dst[i] = (float)R[i];
  for (int i = 0; i < 3; i++) dst[9 + i] = (float)(sign_t * t[i]);
}

// hs::jacobi_cols<M, 9> across the lanes of one wave.  The M rows of A and the 9 rows of V lie in LDS (row-major, 9
// wide: rows 0 .. M-1 are A, rows M .. M+8 are V).  Every lane forms the three sums of a pair over the rows in
// ascending order from broadcast LDS reads, so every lane holds exactly what the single-lane code computes, bit for
// bit, and takes the same decision; the rotation of all M + 9 rows is then one step, one row per lane.  The block is
// one wave, so the barriers are wave-local.
template <int M>
__device__ int wave_jacobi9(double* sh, int lane) {
  constexpr int kRows = M + 9;
  int sweeps = 0;
  while (sweeps < hs::kJacobiMaxSweeps) {
    int rotated = 0;
    for (int p = 0; p < 8; p++)
      for (int q = p + 1; q < 9; q++) {
        double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
        for (int i = 0; i < M; i++) {
          const double x = sh[i * 9 + p], y = sh[i * 9 + q];
          al = al + x * x;
          be = be + y * y;
          ga = ga + x * y;
        }
        const bool skip = ga == 0.0 || fabs(ga) <= hs::kJacobiTol * sqrt(al * be);
        if (!skip) rotated++;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t);
        const double s = c * t;
        __syncthreads();  // every lane has read both columns
        if (!skip && lane < kRows) {
          const double x = sh[lane * 9 + p], y = sh[lane * 9 + q];
          sh[lane * 9 + p] = c * x - s * y;
          sh[lane * 9 + q] = s * x + c * y;
        }
        __syncthreads();
      }
    sweeps++;
    if (!rotated) break;
  }
  return sweeps;
}

// the null vector after wave_jacobi9: V's column under the smallest column of A (hs::jacobi_min_col's order)
template <int M>
__device__ void wave_null_vector(const double* sh, double* v) {
  double n2[9];
  int best = 0;
  for (int j = 0; j < 9; j++) {
    double s = 0.0;
    for (int i = 0; i < M; i++) s = s + sh[i * 9 + j] * sh[i * 9 + j];
    n2[j] = s;
    if (s < n2[best]) best = j;
  }
  for (int i = 0; i < 9; i++) v[i] = sh[(M + i) * 9 + best];
}

}  // namespace

__global__ __launch_bounds__(256) void hs_k_tv_begin(HsTvArgs a) {
  int bad = 0;
  for (int i = threadIdx.x; i < a.n_in_sets * 8; i += kBlock)
    if (a.in_status[a.in_sets[i]] == 0) bad = 1;
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    a.st->bad = bad;
    if (!bad) {
      a.st->n_in_h = 0;
      a.st->n_in_f = 0;
    }
  }
}

// The ascending list of the keys with in_status != 0 (a stable compaction) and its length m.  One block walks the keys
// in chunks of its own size behind a running base, so any n fits one launch: within a chunk a wave's ballot ranks its
// lanes, and the waves' counts in LDS place the wave.  Integer counts only.
__global__ __launch_bounds__(1024) void hs_k_tv_good_list(HsTvArgs a) {
  constexpr int kNt = 1024, kWaves = kNt / 64;
  __shared__ int wcnt[kWaves];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int base = 0;
  for (int c0 = 0; c0 < a.n; c0 += kNt) {
    const int i = c0 + t;
    const bool f = i < a.n && a.in_status[i] != 0;
    const unsigned long long mask = __ballot(f);
    if (lane == 0) wcnt[w] = __popcll(mask);
    __syncthreads();
    int off = 0, tot = 0;
    for (int k = 0; k < kWaves; k++) {
      const int c = wcnt[k];
      if (k < w) off += c;
      tot += c;
    }
    if (f) a.all[base + off + __popcll(mask & ((1ull << lane) - 1ull))] = i;
    base += tot;
    __syncthreads();  // wcnt is rewritten by the next chunk
  }
  if (t == 0) {
    a.st->m = base;
    if (base < 8) a.st->bad = 2;
  }
}

// mvSets (Initializer.cpp:404-432), one lane per set: r = uniform(0, size - 1) from the set's words, sets[it][j] =
// avail[r], avail[r] = avail[size - 1], pop.  avail is never copied: the swap-and-pop rewrites at most eight slots, which
// the lane keeps in registers (the latest override of a slot wins); every other slot is read from `all`.  With m == 8
// the eighth draw is uniform(0, 0) and takes no word, so a set's words are 7 apart.
__global__ __launch_bounds__(64) void hs_k_tv_draw(HsTvArgs a) {
  const int it = blockIdx.x * 64 + threadIdx.x;
  const int m = a.st->m;
  if (it >= a.n_draw || m < 8) return;
  const uint32_t* w = a.words + (size_t)it * (m == 8 ? 7 : 8);
  int slot[8], val[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int last = m - j - 1;
    const int r = last > 0 ? (int)(w[j] % (unsigned)last) : 0;
    int vr = a.all[r], vl = a.all[last];
#pragma unroll
    for (int k = 0; k < j; k++) {
      if (slot[k] == r) vr = val[k];
      if (slot[k] == last) vl = val[k];
    }
    a.draw_out[it * 8 + j] = vr;
    slot[j] = r;
    val[j] = vl;
  }
}

__global__ __launch_bounds__(256) void hs_k_tv_pack(HsTvArgs a) {
  if (a.st->bad) return;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < a.n) {
    const float2 p = a.in1[i], q = a.in2[i];
    a.keys[i] = make_float4(p.x, p.y, q.x, q.y);
    a.status[i] = a.in_status[i] != 0 ? 1 : 0;
  }
  if (i < a.n_in_sets * 8) a.sets[i] = a.in_sets[i];
}

__global__ __launch_bounds__(256) void hs_k_tv_normalize(HsTvArgs a) {
  if (a.st->bad) return;
  __shared__ double sh[kBlock];
  const int t = threadIdx.x;
  const bool second = blockIdx.x == 1;
  double sx = 0.0, sy = 0.0;
  for (int i = t; i < a.n; i += kBlock) {
    const float4 k = a.keys[i];
    sx = sx + (double)(second ? k.z : k.x);
    sy = sy + (double)(second ? k.w : k.y);
  }
  const double SX = block_sum(sx, sh);
  const double SY = block_sum(sy, sh);
  const float meanX = (float)(SX / (double)a.n), meanY = (float)(SY / (double)a.n);
  double dx = 0.0, dy = 0.0;
  for (int i = t; i < a.n; i += kBlock) {
    const float4 k = a.keys[i];
    dx = dx + (double)fabsf((second ? k.z : k.x) - meanX);
    dy = dy + (double)fabsf((second ? k.w : k.y) - meanY);
  }
  const double DX = block_sum(dx, sh);
  const double DY = block_sum(dy, sh);
  if (t == 0) {
    const float devX = (float)(DX / (double)a.n), devY = (float)(DY / (double)a.n);
    float* o = a.norm + 4 * blockIdx.x;
    o[0] = meanX;
    o[1] = meanY;
    o[2] = (float)(1.0 / (double)devX);
    o[3] = (float)(1.0 / (double)devY);
  }
}

__global__ __launch_bounds__(64) void hs_k_tv_hypotheses(HsTvArgs a) {
  if (a.st->bad) return;
  __shared__ double sh[25 * 9];
  const int lane = threadIdx.x;
  const int g = blockIdx.x;  // one wave per (set, model)
  const bool isF = g >= a.ns_h;
  const int set = isF ? g - a.ns_h : g;
  const float m1x = a.norm[0], m1y = a.norm[1], s1x = a.norm[2], s1y = a.norm[3];
  const float m2x = a.norm[4], m2y = a.norm[5], s2x = a.norm[6], s2y = a.norm[7];
  const int M = isF ? 8 : 16;
  if (lane < 8) {
    const int j = lane;
    const float4 k = a.keys[a.sets[set * 8 + j]];
    const float u1 = (k.x - m1x) * s1x, v1 = (k.y - m1y) * s1y;
    const float u2 = (k.z - m2x) * s2x, v2 = (k.w - m2y) * s2y;
    if (!isF) {  // ComputeH21 (:563-589)
      double* r0 = sh + (2 * j) * 9;
      double* r1 = r0 + 9;
      r0[0] = 0.0; r0[1] = 0.0; r0[2] = 0.0;
      r0[3] = (double)(-u1); r0[4] = (double)(-v1); r0[5] = -1.0;
      r0[6] = (double)(v2 * u1); r0[7] = (double)(v2 * v1); r0[8] = (double)v2;
      r1[0] = (double)u1; r1[1] = (double)v1; r1[2] = 1.0;
      r1[3] = 0.0; r1[4] = 0.0; r1[5] = 0.0;
      r1[6] = (double)(-u2 * u1); r1[7] = (double)(-u2 * v1); r1[8] = (double)(-u2);
    } else {     // ComputeF21 (:604-620)
      double* r = sh + j * 9;
      r[0] = (double)(u2 * u1); r[1] = (double)(u2 * v1); r[2] = (double)u2;
      r[3] = (double)(v2 * u1); r[4] = (double)(v2 * v1); r[5] = (double)v2;
      r[6] = (double)u1; r[7] = (double)v1; r[8] = 1.0;
    }
  } else if (lane >= 16 && lane < 25) {  // V = I
    const int i = lane - 16;
    for (int c = 0; c < 9; c++) sh[(M + i) * 9 + c] = i == c ? 1.0 : 0.0;
  }
  __syncthreads();
  if (isF) wave_jacobi9<8>(sh, lane);
  else wave_jacobi9<16>(sh, lane);
  if (lane != 0) return;
  // T1, and T2's entries, as the reference's fp32 matrices hold them
  const double T1[9] = {(double)s1x, 0.0, (double)(-m1x * s1x), 0.0, (double)s1y, (double)(-m1y * s1y), 0.0, 0.0, 1.0};
  const double t2sx = (double)s2x, t2sy = (double)s2y, t2cx = (double)(-m2x * s2x), t2cy = (double)(-m2y * s2y);
  double v[9], tmp[9], Mx[9];
  if (!isF) {
    wave_null_vector<16>(sh, v);
    const double T2inv[9] = {1.0 / t2sx, 0.0, -t2cx / t2sx, 0.0, 1.0 / t2sy, -t2cy / t2sy, 0.0, 0.0, 1.0};
    hs::mul3(T2inv, v, tmp);
    hs::mul3(tmp, T1, Mx);
    hs::inv3(Mx, tmp);
    for (int i = 0; i < 9; i++) {
      a.models[set * 9 + i] = (float)Mx[i];
      a.h12[set * 9 + i] = (float)tmp[i];
    }
  } else {
    wave_null_vector<8>(sh, v);
    // the rank-2 projection: drop the smallest of the three columns of Fpre * V
    double B[9], V[9], n2[3], Fn[9];
    for (int i = 0; i < 9; i++) B[i] = v[i];
    hs::jacobi_cols<3, 3>(B, V);
    const int drop = hs::jacobi_min_col<3, 3>(B, n2);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) {
        double s = 0.0;
        for (int k = 0; k < 3; k++)
          if (k != drop) s = s + B[r * 3 + k] * V[c * 3 + k];
        Fn[r * 3 + c] = s;
      }
    const double T2t[9] = {t2sx, 0.0, 0.0, 0.0, t2sy, 0.0, t2cx, t2cy, 1.0};
    hs::mul3(T2t, Fn, tmp);
    hs::mul3(tmp, T1, Mx);
    for (int i = 0; i < 9; i++) a.models[(kTvMaxSets + set) * 9 + i] = (float)Mx[i];
  }
}

__global__ __launch_bounds__(256) void hs_k_tv_scores(HsTvArgs a) {
  if (a.st->bad) return;
  __shared__ double sh[kBlock];
  const int b = blockIdx.x;
  const bool isF = b >= a.ns_h;
  const int set = isF ? b - a.ns_h : b;
  float M[9], Mi[9];
  for (int i = 0; i < 9; i++) {
    M[i] = a.models[((isF ? kTvMaxSets : 0) + set) * 9 + i];
    Mi[i] = isF ? 0.f : a.h12[set * 9 + i];
  }
  double part = 0.0;
  for (int i = threadIdx.x; i < a.n; i += kBlock) {
    if (!a.status[i]) continue;
    float c1, c2;
    const float4 k = a.keys[i];
    if (isF) score_f(M, k, &c1, &c2);
    else score_h(M, Mi, k, &c1, &c2);
    part = part + (double)c1;
    part = part + (double)c2;
  }
  const double s = block_sum(part, sh);
  if (threadIdx.x == 0) a.scores[(isF ? kTvMaxSets : 0) + set] = (float)s;
}

__global__ __launch_bounds__(256) void hs_k_tv_winners(HsTvArgs a) {
  if (a.st->bad) return;
  __shared__ float sv[kBlock];
  __shared__ int si[kBlock];
  float SH, SF;
  const int bh = block_argmax(a.scores, a.ns_h, sv, si, &SH);
  const int bf = block_argmax(a.scores + kTvMaxSets, a.ns_f, sv, si, &SF);
  const int i = blockIdx.x * kBlock + threadIdx.x;
  bool inh = false, inf_ = false;
  if (i < a.n && a.status[i]) {
    const float4 k = a.keys[i];
    float c1, c2;
    if (bh >= 0) inh = score_h(a.models + bh * 9, a.h12 + bh * 9, k, &c1, &c2);
    if (bf >= 0) inf_ = score_f(a.models + (kTvMaxSets + bf) * 9, k, &c1, &c2);
  }
  if (i < a.n) {
    a.inl[i] = inh ? 1 : 0;
    a.inl[a.n + i] = inf_ ? 1 : 0;
  }
  const int ch = __syncthreads_count(inh);
  const int cf = __syncthreads_count(inf_);
  if (threadIdx.x == 0) {
    if (ch) atomicAdd(&a.st->n_in_h, ch);
    if (cf) atomicAdd(&a.st->n_in_f, cf);
    if (blockIdx.x == 0) {
      a.st->best_h = bh;
      a.st->best_f = bf;
      a.st->SH = SH;
      a.st->SF = SF;
    }
  }
}

__global__ __launch_bounds__(64) void hs_k_tv_decompose(HsTvArgs a) {
  if (a.st->bad) return;
  if (threadIdx.x != 0) return;
  HsTvState* st = a.st;
  st->why = 0;
  st->n_rt = 0;
  st->model = -1;
  const float SH = st->SH, SF = st->SF;
  if (SH == 0.f && SF == 0.f) {
    st->why = hs::HS_TV_NO_SCORE;
    return;
  }
  const float RH = SH / (SH + SF);                                    // :446
  const int model = ((double)RH > 0.40) ? 0 : 1;                      // :449
  st->model = model;
  const double K[9] = {(double)a.fx, 0.0, (double)a.cx, 0.0, (double)a.fy, (double)a.cy, 0.0, 0.0, 1.0};
  double Md[9], tmp[9], A[9], U[9], w[3], Vt[9];
  const float* Mf = a.models + ((model ? kTvMaxSets : 0) + (model ? st->best_f : st->best_h)) * 9;
  for (int i = 0; i < 9; i++) Md[i] = (double)Mf[i];
  if (model == 1) {
    const double Kt[9] = {K[0], 0.0, 0.0, 0.0, K[4], 0.0, K[2], K[5], 1.0};
    hs::mul3(Kt, Md, tmp);                                             // :820
    hs::mul3(tmp, K, A);
    hs::jacobi_svd3(A, U, w, Vt, false);                               // DecomposeE (:1261-1281)
    double t[3] = {U[2], U[5], U[8]};
    const double nt = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    for (int i = 0; i < 3; i++) t[i] = t[i] / nt;
    const double W[9] = {0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
    const double Wt[9] = {0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
    double R1[9], R2[9];
    hs::mul3(U, W, tmp);
    hs::mul3(tmp, Vt, R1);
    if (hs::det3(R1) < 0.0)
      for (int i = 0; i < 9; i++) R1[i] = -R1[i];
    hs::mul3(U, Wt, tmp);
    hs::mul3(tmp, Vt, R2);
    if (hs::det3(R2) < 0.0)
      for (int i = 0; i < 9; i++) R2[i] = -R2[i];
    store_rt(st->rt[0], R1, t, 1.0);                                   // :835-838
    store_rt(st->rt[1], R2, t, 1.0);
    store_rt(st->rt[2], R1, t, -1.0);
    store_rt(st->rt[3], R2, t, -1.0);
    st->n_rt = 4;
    return;
  }
  // ReconstructH (:928-1030)
  const double Kinv[9] = {1.0 / K[0], 0.0, -K[2] / K[0], 0.0, 1.0 / K[4], -K[5] / K[4], 0.0, 0.0, 1.0};
  hs::mul3(Kinv, Md, tmp);
  hs::mul3(tmp, K, A);
  hs::jacobi_svd3(A, U, w, Vt, true);
  const double s = hs::det3(U) * hs::det3(Vt);
  const double d1 = w[0], d2 = w[1], d3 = w[2];
  const float r12 = (float)d1 / (float)d2, r23 = (float)d2 / (float)d3;
  if ((double)r12 < 1.00001 || (double)r23 < 1.00001) {                // :941
    st->why = hs::HS_TV_H_SINGULAR;
    return;
  }
  const double aux1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
  const double aux3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const double x1[4] = {aux1, aux1, -aux1, -aux1};
  const double x3[4] = {aux3, -aux3, aux3, -aux3};
  const double aux_st = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
  const double ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
  const double stheta[4] = {aux_st, -aux_st, -aux_st, aux_st};
  const double aux_sp = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
  const double cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
  const double sphi[4] = {aux_sp, -aux_sp, -aux_sp, aux_sp};
  for (int h = 0; h < 8; h++) {
    const int i = h & 3;
    double Rp[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tp[3];
    if (h < 4) {
      Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
      tp[0] = x1[i] * (d1 - d3); tp[1] = 0.0; tp[2] = -x3[i] * (d1 - d3);
    } else {
      Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1.0; Rp[6] = sphi[i]; Rp[8] = -cphi;
      tp[0] = x1[i] * (d1 + d3); tp[1] = 0.0; tp[2] = x3[i] * (d1 + d3);
    }
    double R[9], t[3];
    hs::mul3(U, Rp, tmp);
    hs::mul3(tmp, Vt, R);
    for (int k = 0; k < 9; k++) R[k] = s * R[k];
    for (int k = 0; k < 3; k++) t[k] = (U[k * 3] * tp[0] + U[k * 3 + 1] * tp[1]) + U[k * 3 + 2] * tp[2];
    const double nt = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    for (int k = 0; k < 3; k++) t[k] = t[k] / nt;
    store_rt(st->rt[h], R, t, 1.0);
  }
  st->n_rt = 8;
}

__global__ __launch_bounds__(256) void hs_k_tv_check_rt(HsTvArgs a) {
  if (a.st->bad) return;
  const int h = blockIdx.y;
  if (h >= a.st->n_rt) return;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const size_t o = (size_t)h * a.n + i;
  const uint8_t* mask = a.rt_inl ? a.rt_inl : a.inl + (size_t)(a.st->model == 1 ? a.n : 0);
  a.rt_pass[o] = 0;
  a.rt_good[o] = 0;
  a.rt_cos[o] = 0.f;
  a.rt_p3d[3 * o] = 0.f;
  a.rt_p3d[3 * o + 1] = 0.f;
  a.rt_p3d[3 * o + 2] = 0.f;
  if (!mask[i]) return;                                                // :1192
  const float* R = a.st->rt[h];
  const float* t = R + 9;
  const float K[9] = {a.fx, 0.f, a.cx, 0.f, a.fy, a.cy, 0.f, 0.f, 1.f};
  // P1 = K[I|0], P2 = K[R|t] (:1150-1159), fp32
  float P1[12], P2[12];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) {
      P1[r * 4 + c] = c < 3 ? K[r * 3 + c] : 0.f;
      const float x0 = c < 3 ? R[c] : t[0], x1 = c < 3 ? R[3 + c] : t[1], x2 = c < 3 ? R[6 + c] : t[2];
      P2[r * 4 + c] = (K[r * 3] * x0 + K[r * 3 + 1] * x1) + K[r * 3 + 2] * x2;
    }
  const float4 k = a.keys[i];
  double A[16], v[4];
  for (int c = 0; c < 4; c++) {                                        // Triangulate (:1079-1082)
    A[c] = (double)(k.x * P1[8 + c] - P1[c]);
    A[4 + c] = (double)(k.y * P1[8 + c] - P1[4 + c]);
    A[8 + c] = (double)(k.z * P2[8 + c] - P2[c]);
    A[12 + c] = (double)(k.w * P2[8 + c] - P2[4 + c]);
  }
  hs::jacobi_null_vector<4, 4>(A, v);
  const float X = (float)(v[0] / v[3]), Y = (float)(v[1] / v[3]), Z = (float)(v[2] / v[3]);
  if (!isfinite(X) || !isfinite(Y) || !isfinite(Z)) return;            // :1201
  // O2 = -R^T t (:1161); parallax (:1208-1214)
  const float O2x = -((R[0] * t[0] + R[3] * t[1]) + R[6] * t[2]);
  const float O2y = -((R[1] * t[0] + R[4] * t[1]) + R[7] * t[2]);
  const float O2z = -((R[2] * t[0] + R[5] * t[1]) + R[8] * t[2]);
  const float n2x = X - O2x, n2y = Y - O2y, n2z = Z - O2z;
  const float dist1 = (float)sqrt(((double)X * (double)X + (double)Y * (double)Y) + (double)Z * (double)Z);
  const float dist2 = (float)sqrt(((double)n2x * (double)n2x + (double)n2y * (double)n2y) + (double)n2z * (double)n2z);
  const double dot = ((double)X * (double)n2x + (double)Y * (double)n2y) + (double)Z * (double)n2z;
  const float cosP = (float)(dot / (double)(dist1 * dist2));
  const bool lowpar = (double)cosP < 0.99998;
  if (Z <= 0.f && lowpar) return;                                      // :1217
  const float X2 = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0];          // :1221
  const float Y2 = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1];
  const float Z2 = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2];
  if (Z2 <= 0.f && lowpar) return;                                     // :1223
  const float th2 = 4.0f;
  const float invZ1 = (float)(1.0 / (double)Z);                        // :1228-1235
  const float im1x = a.fx * X * invZ1 + a.cx, im1y = a.fy * Y * invZ1 + a.cy;
  const float e1 = (im1x - k.x) * (im1x - k.x) + (im1y - k.y) * (im1y - k.y);
  if (e1 > th2) return;
  const float invZ2 = (float)(1.0 / (double)Z2);                       // :1239-1246
  const float im2x = a.fx * X2 * invZ2 + a.cx, im2y = a.fy * Y2 * invZ2 + a.cy;
  const float e2 = (im2x - k.z) * (im2x - k.z) + (im2y - k.w) * (im2y - k.w);
  if (e2 > th2) return;
  a.rt_p3d[3 * o] = X;                                                 // :1248-1257
  a.rt_p3d[3 * o + 1] = Y;
  a.rt_p3d[3 * o + 2] = Z;
  a.rt_cos[o] = cosP;
  a.rt_pass[o] = 1;
  a.rt_good[o] = lowpar ? 1 : 0;
}

__global__ __launch_bounds__(256) void hs_k_tv_select(HsTvArgs a) {
  if (a.st->bad) return;
  const int h = blockIdx.x;
  if (h >= a.st->n_rt) return;
  __shared__ unsigned hist[kBlock];
  __shared__ unsigned ctl[2];
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const uint8_t* pass = a.rt_pass + (size_t)h * a.n;
  int c = 0;
  for (int i = threadIdx.x; i < a.n; i += kBlock) c += pass[i] ? 1 : 0;
  if (c) atomicAdd(&cnt, c);
  __syncthreads();
  const int nGood = cnt;
  float parallax = 0.f;                                                // :1173-1181
  if (nGood > 0) {
    const int idx = nGood - 1 < 50 ? nGood - 1 : 50;
    const float cs = block_select(a.rt_cos + (size_t)h * a.n, 1, pass, a.n, idx, hist, ctl);
    const float ac = (float)acos((double)cs);
    parallax = (float)((double)(ac * 180.f) / 3.1415926535897932384626433832795);
  }
  if (threadIdx.x == 0) {
    a.st->n_good[h] = nGood;
    a.st->parallax[h] = parallax;
  }
}

__global__ __launch_bounds__(256) void hs_k_tv_finish(HsTvArgs a) {
  if (a.st->bad) return;
  HsTvState* st = a.st;
  __shared__ unsigned hist[kBlock];
  __shared__ unsigned ctl[2];
  __shared__ int cnt;
  __shared__ hs::TwoViewPick pick;
  const int t = threadIdx.x;
  if (t == 0) {
    cnt = 0;
    pick.ok = 0;
    pick.why = st->why;
    pick.best = -1;
    if (st->why == 0) {
      const int N = st->model == 1 ? st->n_in_f : st->n_in_h;
      pick = st->model == 1 ? hs::twoview_rule_f(st->n_good, st->parallax, N, 1.0f, 50)
                            : hs::twoview_rule_h(st->n_good, st->parallax, N, 1.0f, 50);
    }
  }
  __syncthreads();
  const int best = pick.best;
  int ok = pick.ok, why = pick.why;
  const uint8_t* good = a.rt_good + (size_t)(best < 0 ? 0 : best) * a.n;
  const float* p3 = a.rt_p3d + (size_t)(best < 0 ? 0 : best) * a.n * 3;
  float med = 0.f;
  int ntri = 0;
  if (ok) {
    int c = 0;
    for (int i = t; i < a.n; i += kBlock) c += good[i] ? 1 : 0;
    if (c) atomicAdd(&cnt, c);
    __syncthreads();
    ntri = cnt;
    if (ntri == 0) {  // nothing to take a median of: the reference would index an empty vector
      ok = 0;
      why = hs::HS_TV_NO_WINNER;
    } else {
      med = block_select(p3 + 2, 3, good, a.n, (ntri - 1) / 2, hist, ctl);  // :1283-1297
    }
  }
  for (int i = t; i < a.n; i += kBlock) {
    const bool g = ok && good[i];
    a.tri[i] = g ? 1 : 0;
    const float x = g ? p3[3 * i] / med : 0.f, y = g ? p3[3 * i + 1] / med : 0.f, z = g ? p3[3 * i + 2] / med : 0.f;
    a.p3d[3 * i] = x;
    a.p3d[3 * i + 1] = y;
    a.p3d[3 * i + 2] = z;
    a.z[i] = z;
  }
  if (t == 0) {
    hs_twoview_result r;
    r.ok = ok;
    r.why = why;
    r.model = st->model;
    r.best_h = st->best_h;
    r.best_f = st->best_f;
    r.n_inliers = st->model < 0 ? 0 : (st->model == 1 ? st->n_in_f : st->n_in_h);
    r.SH = st->SH;
    r.SF = st->SF;
    for (int i = 0; i < 9; i++) r.R[i] = ok ? st->rt[best][i] : 0.f;
    for (int i = 0; i < 3; i++) r.t[i] = ok ? st->rt[best][9 + i] / med : 0.f;
    r.n_good = best >= 0 ? st->n_good[best] : 0;
    r.parallax_deg = best >= 0 ? st->parallax[best] : 0.f;
    r.n_triangulated = ntri;
    r.median_depth = med;
    r.best_rt = best;
    r.n_rt = st->n_rt;
    for (int i = 0; i < 6; i++) r.reserved[i] = 0;
    st->res = r;
  }
}
