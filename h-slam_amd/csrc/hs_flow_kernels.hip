// hs_flow_kernels.hip — the kernels of include/hs_flow.h.  The level images are stored with a 15 px reflected
// border and the derivative levels with a 15 px zero border, so the tracker's gathers need no border logic: a
// window's top-left tap passes the float bounds test (>= -15, < size) before it becomes an index, and the window
// then reaches at most 15 px outside on either side.  Built with -ffp-contract=off: every float operation of the
// contract is one rounded operation.
#include "hs_flow_kernels.h"

namespace {

__device__ __forceinline__ int refl(int i, int n) {  // reflect-101; valid for -(n-1) <= i <= 2n-2
  i = i < 0 ? -i : i;
  return i >= n ? 2 * n - 2 - i : i;
}

// v + (v of the lane a DPP control selects); a lane without a source, or in a row the mask leaves out, adds 0
template <int kCtrl, int kRowMask>
__device__ __forceinline__ long long dpp_add(long long v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)v, kCtrl, kRowMask, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(v >> 32), kCtrl, kRowMask, 0xf, false);
  return v + (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// Exact sum over the wave, the same value in every lane (integer adds: no order dependence).  All 64 lanes must be
// active.  Register-to-register DPP steps instead of 64-bit shuffles through the LDS crossbar: the reduction is on
// every iteration's critical path.  Quads, then each row of 16 into its lane 15, rows 0 / 2 into rows 1 / 3, row 1
// into rows 2 and 3: lane 63 holds the total.
__device__ __forceinline__ long long wave_sum(long long v) {
  v = dpp_add<0xb1, 0xf>(v);   // quad_perm:[1,0,3,2]
  v = dpp_add<0x4e, 0xf>(v);   // quad_perm:[2,3,0,1]
  v = dpp_add<0x114, 0xf>(v);  // row_shr:4
  v = dpp_add<0x118, 0xf>(v);  // row_shr:8
  v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
  v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), 63);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// an exact integer of up to 53 bits to float, rounded once
__device__ __forceinline__ float to_float(long long v) { return (float)(double)v; }

// correctly rounded float sqrt and division by way of double (53 >= 2 * 24 + 2: the second rounding is innocuous)
__device__ __forceinline__ float sqrt_rn(float x) { return (float)sqrt((double)x); }
__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }

// the contract's bounds test on the floats: NaN and huge values fail it, and only what passes becomes an index
__device__ __forceinline__ bool inside(float x, float y, int w, int h) {
  return x >= -(float)kFlowWin && x < (float)w && y >= -(float)kFlowWin && y < (float)h;
}

struct Weights {
  int ix, iy;  // floor of the point
  int w00, w01, w10, w11;
};

__device__ __forceinline__ Weights make_weights(float x, float y) {
  Weights r;
  const float fx = floorf(x), fy = floorf(y);
  r.ix = (int)fx;
  r.iy = (int)fy;
  const float a = x - fx, b = y - fy;
  r.w00 = (int)rintf((1.f - a) * (1.f - b) * 16384.f);
  r.w01 = (int)rintf(a * (1.f - b) * 16384.f);
  r.w10 = (int)rintf((1.f - a) * b * 16384.f);
  r.w11 = 16384 - r.w00 - r.w01 - r.w10;
  return r;
}

// (sum taps * iw + 256) >> 9 of the padded image at tap (tx, ty), level coordinates
__device__ __forceinline__ int sample_img(const uint8_t* img, int stride, int tx, int ty, const Weights& w) {
  const uint8_t* p = img + (size_t)(ty + kFlowPad) * stride + (tx + kFlowPad);
  const int v = (int)p[0] * w.w00 + (int)p[1] * w.w01 + (int)p[stride] * w.w10 + (int)p[stride + 1] * w.w11;
  return (v + 256) >> 9;
}

}  // namespace

__global__ __launch_bounds__(256) void hs_k_flow_pack_xy(int n, const float* x, const float* y, float2* xy) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) xy[i] = make_float2(x[i], y[i]);
}

__global__ __launch_bounds__(256) void hs_k_flow_pad(HsFlowPadArgs a) {
  const int pw = a.w + 2 * kFlowPad, ph = a.h + 2 * kFlowPad;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pw * ph) return;
  const int Y = i / pw, X = i - Y * pw;
  a.dst[i] = a.src[(size_t)refl(Y - kFlowPad, a.h) * a.w + refl(X - kFlowPad, a.w)];
}

__global__ __launch_bounds__(256) void hs_k_flow_pyrdown(HsFlowDownArgs a) {
  const int pw = a.dw + 2 * kFlowPad, ph = a.dh + 2 * kFlowPad;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pw * ph) return;
  const int Y = i / pw, X = i - Y * pw;
  const int x = refl(X - kFlowPad, a.dw), y = refl(Y - kFlowPad, a.dh);
  // taps 2x-2 .. 2x+2 lie in [-2, sw+1]: the source's reflected border holds r() of them
  const int ss = a.sw + 2 * kFlowPad;
  const uint8_t* p = a.src + (size_t)(2 * y - 2 + kFlowPad) * ss + (2 * x - 2 + kFlowPad);
  int sum = 0;
#pragma unroll
  for (int r = 0; r < 5; r++) {
    const int kr = r == 0 || r == 4 ? 1 : (r == 2 ? 6 : 4);
    const uint8_t* q = p + (size_t)r * ss;
    sum += kr * ((int)q[0] + 4 * (int)q[1] + 6 * (int)q[2] + 4 * (int)q[3] + (int)q[4]);
  }
  a.dst[i] = (uint8_t)((sum + 128) >> 8);
}

__global__ __launch_bounds__(256) void hs_k_flow_scharr(HsFlowScharrArgs a) {
  const int pw = a.w + 2 * kFlowPad, ph = a.h + 2 * kFlowPad;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pw * ph) return;
  const int Y = i / pw, X = i - Y * pw;
  short2 d = make_short2(0, 0);
  if (X >= kFlowPad && X < kFlowPad + a.w && Y >= kFlowPad && Y < kFlowPad + a.h) {
    // the 3 x 3 neighbourhood lies inside the padded image, whose border holds r() of the taps
    const uint8_t* p = a.img + i;
    int t0[3], t1[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const int up = p[c - 1 - pw], mid = p[c - 1], dn = p[c - 1 + pw];
      t0[c] = 3 * (up + dn) + 10 * mid;
      t1[c] = dn - up;
    }
    d.x = (short)(t0[2] - t0[0]);
    d.y = (short)(3 * (t1[2] + t1[0]) + 10 * t1[1]);
  }
  a.deriv[i] = d;
}

// One wave per point, four points per block; the level loop runs inside.  The 225 window pixels are spread four per
// lane (lane, lane + 64, lane + 128, lane + 192 < 225) and each pixel's (I, Ix, Iy) stays in registers over the
// iterations.  The five sums are exact 64-bit integer reductions that leave the same value in every lane, so all
// lanes run the same scalar float arithmetic and the control flow is uniform over the wave.
__global__ __launch_bounds__(256) void hs_k_flow_lk(HsFlowLkArgs a) {
  const int lane = threadIdx.x & 63;
  const int pt = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pt >= a.n) return;  // the whole wave

  int wx[4], wy[4];
  bool act[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int idx = lane + 64 * k;
    act[k] = idx < kFlowWin * kFlowWin;
    wy[k] = act[k] ? idx / kFlowWin : 0;
    wx[k] = act[k] ? idx - wy[k] * kFlowWin : 0;
  }

  const float half = 7.f;
  const float2 prev = a.prev_xy[pt];
  float ox = 0.f, oy = 0.f, err = 0.f;
  int status = 1;
  unsigned iters = 0;
  const int top = a.lv.n - 1;
  for (int l = top; l >= 0; --l) {
    const int w = a.lv.w[l], h = a.lv.h[l], stride = w + 2 * kFlowPad;
    const uint8_t* I_img = a.prev_img + a.lv.off[l];
    const short2* D_img = a.prev_deriv + a.lv.off[l];
    const uint8_t* J_img = a.next_img + a.lv.off[l];
    const float s = 1.f / (float)(1 << l);
    float px = prev.x * s, py = prev.y * s;
    float gx, gy;
    if (l == top) {
      if (a.init_xy) {
        const float2 g0 = a.init_xy[pt];
        gx = g0.x * s;
        gy = g0.y * s;
      } else {
        gx = px;
        gy = py;
      }
    } else {
      gx = ox * 2.f;
      gy = oy * 2.f;
    }
    ox = gx;
    oy = gy;
    px -= half;
    py -= half;
    if (!inside(px, py, w, h)) {
      if (l == 0) status = 0;
      continue;
    }
    const Weights pw = make_weights(px, py);
    int Iv[4], Ix[4], Iy[4];
    long long s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      Iv[k] = Ix[k] = Iy[k] = 0;
      if (act[k]) {
        const int tx = pw.ix + wx[k], ty = pw.iy + wy[k];
        Iv[k] = sample_img(I_img, stride, tx, ty, pw);
        const short2* d = D_img + (size_t)(ty + kFlowPad) * stride + (tx + kFlowPad);
        const short2 d00 = d[0], d01 = d[1], d10 = d[stride], d11 = d[stride + 1];
        Ix[k] = ((int)d00.x * pw.w00 + (int)d01.x * pw.w01 + (int)d10.x * pw.w10 + (int)d11.x * pw.w11 + 8192) >> 14;
        Iy[k] = ((int)d00.y * pw.w00 + (int)d01.y * pw.w01 + (int)d10.y * pw.w10 + (int)d11.y * pw.w11 + 8192) >> 14;
        s11 += Ix[k] * Ix[k];  // |Ix| <= 4080: a product fits 25 bits
        s12 += Ix[k] * Iy[k];
        s22 += Iy[k] * Iy[k];
      }
    }
    const float scale = 1.f / (float)(1 << 20);
    const float A11 = to_float(wave_sum(s11)) * scale;
    const float A12 = to_float(wave_sum(s12)) * scale;
    const float A22 = to_float(wave_sum(s22)) * scale;
    float D = A11 * A22 - A12 * A12;
    const float dA = A11 - A22;
    const float min_eig = div_rn(A22 + A11 - sqrt_rn(dA * dA + 4.f * A12 * A12), 450.f);
    if ((double)min_eig < 1e-4 || D < 1.1920928955078125e-07f) {
      if (l == 0) status = 0;
      continue;
    }
    D = div_rn(1.f, D);

    float qx = gx - half, qy = gy - half;
    float pdx = 0.f, pdy = 0.f;
    for (int j = 0; j < kFlowIters; j++) {
      if (!inside(qx, qy, w, h)) {
        if (l == 0) status = 0;
        break;
      }
      const Weights qw = make_weights(qx, qy);
      long long sb1 = 0, sb2 = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (act[k]) {
          const int diff = sample_img(J_img, stride, qw.ix + wx[k], qw.iy + wy[k], qw) - Iv[k];  // |diff| <= 8160
          sb1 += diff * Ix[k];
          sb2 += diff * Iy[k];
        }
      }
      const float b1 = to_float(wave_sum(sb1)) * scale;
      const float b2 = to_float(wave_sum(sb2)) * scale;
      const float dx = (A12 * b2 - A22 * b1) * D;
      const float dy = (A12 * b1 - A11 * b2) * D;
      iters++;
      qx += dx;
      qy += dy;
      ox = qx + half;
      oy = qy + half;
      if ((double)dx * (double)dx + (double)dy * (double)dy <= 0.01 * 0.01) break;
      if (j > 0 && fabs((double)(dx + pdx)) < 0.01 && fabs((double)(dy + pdy)) < 0.01) {
        ox -= dx * 0.5f;
        oy -= dy * 0.5f;
        break;
      }
      pdx = dx;
      pdy = dy;
    }

    if (l == 0 && status) {
      const float ex = ox - half, ey = oy - half;
      if (!inside(ex, ey, w, h)) {
        status = 0;
      } else {
        const Weights ew = make_weights(ex, ey);
        long long se = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          if (act[k]) {
            const int diff = sample_img(J_img, stride, ew.ix + wx[k], ew.iy + wy[k], ew) - Iv[k];
            se += diff < 0 ? -diff : diff;
          }
        }
        err = to_float(wave_sum(se)) * (1.f / 7200.f);
      }
    }
  }

  if (lane == 0) {
    const int good = status && err < a.max_l1_error;
    a.xy[pt] = make_float2(ox, oy);
    a.status[pt] = (uint8_t)status;
    a.err[pt] = err;
    a.good[pt] = (uint8_t)good;
    if (good) atomicAdd(a.n_good, 1);
    if (iters) atomicAdd(a.n_iters, (unsigned long long)iters);
  }
}

// hs_flow_mean_flow on the device, bit for bit.  The norms of a chunk of keys are made in parallel into LDS; the
// reference's accumulate into an int, acc = (int)((float)acc + norm), rounds the float sum before it truncates, so it
// is not associative and stays one ordered chain: lane 0 walks the chunk in key order.  A key that is not good is stored
// as -1 (a norm is never negative) and leaves acc alone through a select, not a branch, so the chain's LDS reads (four
// keys each) do not wait for the chain.
__global__ __launch_bounds__(256) void hs_k_flow_mean(HsFlowMeanArgs a) {
  constexpr int kChunk = 1024;
  __shared__ float4 norm4[kChunk / 4];
  float* norm = reinterpret_cast<float*>(norm4);
  const int t = threadIdx.x;
  int acc = 0, count = 0;
  for (int c0 = 0; c0 < a.n; c0 += kChunk) {
    for (int k = t; k < kChunk; k += 256) {
      const int i = c0 + k;
      float v = -1.f;
      if (i < a.n && a.good[i]) {
        const float2 p = a.prev_xy[i], q = a.xy[i];
        const float dx = p.x - q.x, dy = p.y - q.y;
        v = (float)sqrt((double)dx * dx + (double)dy * dy);
      }
      norm[k] = v;
    }
    __syncthreads();
    if (t == 0) {
      const int len4 = ((a.n - c0 < kChunk ? a.n - c0 : kChunk) + 3) / 4;
#pragma unroll 4
      for (int k = 0; k < len4; k++) {
        const float4 v = norm4[k];
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int next = (int)((float)acc + e[j]);
          const bool g = !(e[j] < 0.f);
          acc = g ? next : acc;
          count += g ? 1 : 0;
        }
      }
    }
    __syncthreads();  // the next chunk rewrites the LDS
  }
  if (t == 0) *a.mean = (float)acc / (float)count;  // 0 / 0: NaN with no good key
}
