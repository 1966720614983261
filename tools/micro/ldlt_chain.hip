// ldlt_chain.hip — the product's panel LDLT (hs_k_solve's ldlt_solve_blocked + ldlt_backward) against the form it
// had before the panel chain's instruction count was cut (kept here as ldlt_solve_blocked_form<1>: the main loop
// through panel_coop, with the masked carry and the pivots published from the uniform copies), in one binary, on
// random SPD systems scaled like the solve's S H S (unit diagonal), against a host LDLT with the same dead-pivot
// rule (reciprocal 0 for |d| <= DBL_MIN).
//   sizes n = 12, 20, 36, 60, 68 (3, 5, 9, 15, 17 panels; 60: the largest with clamped lanes, 68: rows 64-67);
//   one system per size >= 20 with an exact zero pivot in the last panel (row and column n - 2 zero): the guard must
//   give a finite x with x[n - 2] = 0;
//   cycles (clock64, best of reps) and wall-clock µs of factor + backward for both forms.
// A measuring tool, not a test.
// build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 -I../../h-slam_amd/csrc -o ldlt_chain ldlt_chain.hip
#include "../../h-slam_amd/csrc/hs_ba_kernels.hip"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {
constexpr int MD = HS_MAXDIM;

// panel_chain without the dead-pivot guard on the reciprocal (wrong for a dead pivot): a probe for what the guard's
// compare and selects cost per phase, never a candidate for the product as it stands
__device__ __forceinline__ double panel_chain_noguard(const double a[4], double yr, int l, int base, double lw[4], double ls[4]) {
  double pr[4] = {a[0], a[1], a[2], a[3]};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const double d = hs_solve::readlane_f64(pr[j], base + j);
    double dinv = __builtin_amdgcn_rcp(d);
    dinv = __builtin_fma(dinv, __builtin_fma(-d, dinv, 1.0), dinv);
    const double ydj = hs_solve::readlane_f64(yr, base + j);
    double q[4];
#pragma unroll
    for (int jp = j + 1; jp < 4; jp++) q[jp] = hs_solve::readlane_f64(pr[j], base + jp);
    lw[j] = pr[j];
    ls[j] = l > j ? pr[j] * dinv : 0.0;
#pragma unroll
    for (int jp = j + 1; jp < 4; jp++) pr[jp] = __builtin_fma(-(pr[j] * q[jp]), dinv, pr[jp]);
    yr = __builtin_fma(-ls[j], ydj, yr);
  }
  return yr;
}

// ldlt_solve_blocked with the main loop's panel in another form: same prologue, trailing tiles and backward pass.
//   kForm 1: the previous form (panel_coop, publishing as the prologue does);  kForm 2: the product's loop with
//   panel_chain_noguard (the probe)
template <int kForm>
__device__ __forceinline__ void ldlt_solve_blocked_form(const double* M, double* LT, double* W, double* yv, int n, int tid) {
  const int nb = n >> 2;
  double* PBq = W;
  double* LWb = W + 8 * MD;
  double* Dv = W + 24 * MD;
  double* yf = W + 25 * MD;
  const bool pw = tid < 64;
  const int u = tid - 64;
  int trp = 0;
  while ((trp + 1) * (trp + 2) / 2 <= u) trp++;
  const int tr = 2 + trp, tc = 2 + (u - trp * (trp + 1) / 2);
  const bool tile = !pw && tr < nb;
  double v[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int c = 0; c < 4; c++) v[i][c] = tile ? M[(4 * tr + i) * n + 4 * tc + c] : 0.0;
  if (tid < n)
#pragma unroll
    for (int c = 0; c < 4; c++) PBq[4 * MD + tid * 4 + c] = M[tid * n + 4 + c];
  if (pw) {
    const int r = min(tid, n - 1);
    double a4[4];
#pragma unroll
    for (int c = 0; c < 4; c++) a4[c] = M[r * n + c];
    Panel4 P;
    PanelOut o;
    panel_coop(a4, yv[r], tid, P, o);
    if (tid < n) panel_row_store(o, P, tid, tid, 0, LWb, LT, Dv, yf, yv);
    if (tid + 64 < n) {
      const int r2 = tid + 64;
#pragma unroll
      for (int c = 0; c < 4; c++) a4[c] = M[r2 * n + c];
      panel_row_uniform(a4, yv[r2], P, o);
      panel_row_store(o, P, r2, r2, 0, LWb, LT, Dv, yf, yv);
    }
  }
  __syncthreads();
  const int rw = min(tid + 4, n - 1);
  double lwc[4] = {0.0, 0.0, 0.0, 0.0}, ycar = 0.0;
  if (pw) {
#pragma unroll
    for (int j = 0; j < 4; j++) lwc[j] = LWb[j * MD + rw];
    ycar = yv[rw];
  }
  for (int k = 0; k + 1 < nb; k++) {
    const int K0 = 4 * (k + 1);
    const double* LSk = LT + 4 * k * hs_solve::LSTR;
    if (pw) {
      const double* PBc = PBq + ((k + 1) & 1) * 4 * MD;
      const double4 pb = *reinterpret_cast<const double4*>(PBc + rw * 4);
      double a4[4] = {pb.x, pb.y, pb.z, pb.w};
      double lsd[4][4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const double4 q4 = *reinterpret_cast<const double4*>(LSk + j * hs_solve::LSTR + K0);
        lsd[0][j] = q4.x;
        lsd[1][j] = q4.y;
        lsd[2][j] = q4.z;
        lsd[3][j] = q4.w;
      }
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int c = 0; c < 4; c++) a4[c] = __builtin_fma(-lwc[j], lsd[c][j], a4[c]);
      const int l = tid - 4 * k;
      if (kForm == 1) {
        Panel4 P;
        PanelOut o;
        panel_coop(a4, ycar, l, P, o, 4 * k);
        if (l >= 0 && tid + 4 < n) {
#pragma unroll
          for (int j = 0; j < 4; j++) LT[(K0 + j) * hs_solve::LSTR + rw] = o.ls[j];
          if (l < 4) {
            Dv[rw] = l == 0 ? P.d[0] : l == 1 ? P.d[1] : l == 2 ? P.d[2] : P.d[3];
            yf[rw] = o.yr;
          }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) lwc[j] = o.lw[j];
        ycar = o.yr;
      } else {
        double ls[4];
        ycar = panel_chain_noguard(a4, ycar, l, 4 * k, lwc, ls);
        if (l >= 0 && tid + 4 < n) {
#pragma unroll
          for (int j = 0; j < 4; j++) LT[(K0 + j) * hs_solve::LSTR + rw] = ls[j];
          if (l < 4) {
            const double dlo = (tid & 1) ? lwc[1] : lwc[0], dhi = (tid & 1) ? lwc[3] : lwc[2];
            Dv[rw] = (tid & 2) ? dhi : dlo;
            yf[rw] = ycar;
          }
        }
      }
    } else if (tile && tc >= k + 2) {
      double lw[4][4], ls[4][4], dk[4];
#pragma unroll
      for (int j = 0; j < 4; j++) dk[j] = Dv[4 * k + j];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const double4 r4 = *reinterpret_cast<const double4*>(LSk + j * hs_solve::LSTR + 4 * tr);
        const double4 c4 = *reinterpret_cast<const double4*>(LSk + j * hs_solve::LSTR + 4 * tc);
        lw[0][j] = r4.x * dk[j];
        lw[1][j] = r4.y * dk[j];
        lw[2][j] = r4.z * dk[j];
        lw[3][j] = r4.w * dk[j];
        ls[0][j] = c4.x;
        ls[1][j] = c4.y;
        ls[2][j] = c4.z;
        ls[3][j] = c4.w;
      }
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int c = 0; c < 4; c++) v[i][c] = __builtin_fma(-lw[i][j], ls[c][j], v[i][c]);
      if (tc == k + 2) {
        double* PBn = PBq + (k & 1) * 4 * MD;
#pragma unroll
        for (int i = 0; i < 4; i++)
          *reinterpret_cast<double4*>(PBn + (4 * tr + i) * 4) = make_double4(v[i][0], v[i][1], v[i][2], v[i][3]);
      }
    }
    __syncthreads();
  }
  hs_solve::ldlt_backward(LT, W, yv, n, tid, nullptr);
}

// mode 0: the product; mode 1: the previous form; mode 2: the no-guard probe.  n is a multiple of 4, 8 <= n <= MD.
__global__ __launch_bounds__(512) void k_solve(const double* Mg, const double* bg, double* xg, int n, int mode, int reps,
                                               long long* cyc) {
  __shared__ double A[MD * MD], LTs[MD * hs_solve::LSTR], Ws[LDLT_SCRATCH], y[MD];
  const int tid = threadIdx.x;
  long long best = 1LL << 62, bestw = 1LL << 62;
  for (int r = 0; r < reps; r++) {
    for (int q = tid; q < n * n; q += 512) A[q] = Mg[q];
    for (int q = tid; q < MD * hs_solve::LSTR; q += 512) LTs[q] = 0.0;
    if (tid < n) y[tid] = bg[tid];
    __syncthreads();
    const long long c0 = clock64(), w0 = wall_clock64();
    if (mode == 0) ldlt_solve_blocked(A, LTs, Ws, y, n, tid, nullptr, 0);
    else if (mode == 1) ldlt_solve_blocked_form<1>(A, LTs, Ws, y, n, tid);
    else ldlt_solve_blocked_form<2>(A, LTs, Ws, y, n, tid);
    __syncthreads();
    const long long c1 = clock64(), w1 = wall_clock64();
    if (c1 - c0 < best) best = c1 - c0;
    if (w1 - w0 < bestw) bestw = w1 - w0;
    __syncthreads();
  }
  if (tid < n) xg[tid] = y[tid];
  if (tid == 0) {
    cyc[0] = best;
    cyc[1] = bestw;
  }
}
}  // namespace

#define CK(x)                                                      \
  do {                                                             \
    hipError_t e_ = (x);                                           \
    if (e_ != hipSuccess) {                                        \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); \
      return 1;                                                    \
    }                                                              \
  } while (0)

int main(int argc, char** argv) {
  const int reps = argc > 1 ? std::atoi(argv[1]) : 20;
  int khz = 0;
  CK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0));
  double *dM, *db, *dx;
  long long* dc;
  CK(hipMalloc(&dM, sizeof(double) * MD * MD));
  CK(hipMalloc(&db, sizeof(double) * MD));
  CK(hipMalloc(&dx, sizeof(double) * MD));
  CK(hipMalloc(&dc, sizeof(long long) * 2));
  std::srand(7);
  const int sizes[5] = {12, 20, 36, 60, 68};
  int bad = 0;
  for (int si = 0; si < 5; si++)
    for (int dead = 0; dead < 2; dead++) {
      const int n = sizes[si];
      if (n > MD || (dead && n < 20)) continue;
      // SPD, scaled to a unit diagonal like S H S: B B^T + 0.1 n I, then D^-1/2 . D^-1/2
      std::vector<double> B((size_t)n * n), H((size_t)n * n), b(n), x(n);
      for (auto& v : B) v = (std::rand() / (double)RAND_MAX - 0.5);
      for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) {
          double s = r == c ? 0.1 * n : 0.0;
          for (int k = 0; k < n; k++) s += B[r * n + k] * B[c * n + k];
          H[r * n + c] = s;
        }
      for (int r = 0; r < n; r++) b[r] = std::rand() / (double)RAND_MAX - 0.5;
      std::vector<double> sq(n);
      for (int r = 0; r < n; r++) sq[r] = 1.0 / std::sqrt(H[r * n + r]);
      for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) H[r * n + c] *= sq[r] * sq[c];
      const int zr = n - 2;  // the dead row: zero row and column, so its pivot is exactly 0 whatever the rounding
      if (dead)
        for (int c = 0; c < n; c++) H[zr * n + c] = H[c * n + zr] = 0.0;
      // host reference: unpivoted LDLT in fp64, reciprocal 0 for a dead pivot
      std::vector<double> L((size_t)n * n, 0.0), D(n), Di(n), z(b);
      for (int j = 0; j < n; j++) {
        double d = H[j * n + j];
        for (int k = 0; k < j; k++) d -= L[j * n + k] * L[j * n + k] * D[k];
        D[j] = d;
        Di[j] = std::fabs(d) > DBL_MIN ? 1.0 / d : 0.0;
        L[j * n + j] = 1.0;
        for (int r = j + 1; r < n; r++) {
          double s = H[r * n + j];
          for (int k = 0; k < j; k++) s -= L[r * n + k] * L[j * n + k] * D[k];
          L[r * n + j] = s * Di[j];
        }
      }
      for (int r = 0; r < n; r++)
        for (int k = 0; k < r; k++) z[r] -= L[r * n + k] * z[k];
      for (int r = 0; r < n; r++) z[r] *= Di[r];
      for (int r = n - 1; r >= 0; r--) {
        x[r] = z[r];
        for (int k = r + 1; k < n; k++) x[r] -= L[k * n + r] * x[k];
      }
      CK(hipMemcpy(dM, H.data(), sizeof(double) * n * n, hipMemcpyHostToDevice));
      CK(hipMemcpy(db, b.data(), sizeof(double) * n, hipMemcpyHostToDevice));
      std::vector<double> g[3];
      for (int mode = 0; mode < (dead ? 2 : 3); mode++) {  // the probe has no dead-pivot rule
        hipLaunchKernelGGL(k_solve, dim3(1), dim3(512), 0, 0, dM, db, dx, n, mode, reps, dc);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        g[mode].resize(n);
        long long cy[2];
        CK(hipMemcpy(g[mode].data(), dx, sizeof(double) * n, hipMemcpyDeviceToHost));
        CK(hipMemcpy(cy, dc, sizeof(cy), hipMemcpyDeviceToHost));
        double en = 0, xn = 0;
        bool finite = true;
        for (int r = 0; r < n; r++) {
          en += (g[mode][r] - x[r]) * (g[mode][r] - x[r]);
          xn += x[r] * x[r];
          finite = finite && std::isfinite(g[mode][r]);
        }
        const bool dead_ok = !dead || g[mode][zr] == 0.0;
        const bool same = mode == 0 || std::memcmp(g[0].data(), g[1].data(), sizeof(double) * n) == 0;
        const double rel = std::sqrt(en / xn);
        if (!finite || !dead_ok || !(rel < 1e-9)) bad++;
        std::printf(
            "{\"n\": %d, \"dead_pivot\": %d, \"form\": \"%s\", \"cycles\": %lld, \"us\": %.3f, \"rel_err\": %.3e, "
            "\"finite\": %s, \"dead_x_zero\": %s, \"x_bit_equal_to_product\": %s}\n",
            n, dead, mode == 0 ? "product" : mode == 1 ? "previous" : "probe: no guard", cy[0], cy[1] * 1e3 / (khz > 0 ? khz : 100000), rel,
            finite ? "true" : "false", dead_ok ? "true" : "false", same ? "true" : "false");
      }
    }
  (void)hipFree(dM);
  (void)hipFree(db);
  (void)hipFree(dx);
  (void)hipFree(dc);
  return bad ? 2 : 0;
}
