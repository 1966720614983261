// hs_jacobi.h — the one small dense factorization of the two-view fit (include/hs_twoview.h): a one-sided cyclic
// Jacobi (Hestenes) in fp64, written once for the device kernels (hs_twoview_kernels.hip) and the host
// (tests/c/twoview_main.cpp runs this very code against numpy.linalg.svd).
//
// jacobi_cols<M, N>(A, V) rotates pairs of columns of the row-major M x N matrix A until they are mutually orthogonal
// and accumulates the rotations in the N x N matrix V (V starts as the identity), so that on return A_in * V = A_out,
// the columns of A_out are sigma_j * u_j and the columns of V are the right singular vectors.  M < N is allowed: the
// surplus columns go to (rounding) zero and their V columns span the null space.
//
// Bit-reproducible by construction: the pair order is fixed (p = 0 .. N-2, q = p+1 .. N-1), every sum runs over the
// rows in ascending order, and the stopping rule is fixed: a pair is skipped when its columns' dot product g satisfies
// g == 0 or |g| <= 2^-50 * sqrt(|a_p|^2 |a_q|^2); the sweeps end after the first sweep that rotated nothing, or after
// kJacobiMaxSweeps (a column that is pure rounding noise never becomes orthogonal to the rest; rotating it moves V by
// less than one ulp).  No fused multiply-add: the library and the test program are built with -ffp-contract=off.
#pragma once
#include <math.h>

#ifndef HS_HD
#ifdef __HIPCC__
#define HS_HD __host__ __device__
#else
#define HS_HD
#endif
#endif

namespace hs {

constexpr int kJacobiMaxSweeps = 16;
constexpr double kJacobiTol = 8.8817841970012523e-16;  // 2^-50

template <int M, int N>
HS_HD inline int jacobi_cols(double* A, double* V) {
  for (int i = 0; i < N; i++)
    for (int j = 0; j < N; j++) V[i * N + j] = i == j ? 1.0 : 0.0;
  int sweeps = 0;
  while (sweeps < kJacobiMaxSweeps) {
    int rotated = 0;
    for (int p = 0; p < N - 1; p++)
      for (int q = p + 1; q < N; q++) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int i = 0; i < M; i++) {
          const double a = A[i * N + p], b = A[i * N + q];
          al = al + a * a;
          be = be + b * b;
          ga = ga + a * b;
        }
        if (ga == 0.0 || fabs(ga) <= kJacobiTol * sqrt(al * be)) continue;
        rotated++;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t);
        const double s = c * t;
        for (int i = 0; i < M; i++) {
          const double a = A[i * N + p], b = A[i * N + q];
          A[i * N + p] = c * a - s * b;
          A[i * N + q] = s * a + c * b;
        }
        for (int i = 0; i < N; i++) {
          const double a = V[i * N + p], b = V[i * N + q];
          V[i * N + p] = c * a - s * b;
          V[i * N + q] = s * a + c * b;
        }
      }
    sweeps++;
    if (!rotated) break;
  }
  return sweeps;
}

// squared norms of the columns of A (rows ascending); returns the lowest index that attains the minimum
template <int M, int N>
HS_HD inline int jacobi_min_col(const double* A, double* norm2) {
  int best = 0;
  for (int j = 0; j < N; j++) {
    double s = 0.0;
    for (int i = 0; i < M; i++) s = s + A[i * N + j] * A[i * N + j];
    norm2[j] = s;
    if (s < norm2[best]) best = j;
  }
  return best;
}

// the right singular vector of the smallest singular value of the M x N matrix A (destroyed); out[N]
template <int M, int N>
HS_HD inline void jacobi_null_vector(double* A, double* out) {
  double V[N * N], n2[N];
  jacobi_cols<M, N>(A, V);
  const int j = jacobi_min_col<M, N>(A, n2);
  for (int i = 0; i < N; i++) out[i] = V[i * N + j];
}

// 3 x 3 singular value decomposition A = U diag(w) Vt, w descending (a stable order: of equal values the lower column
// first).  U's columns are the normalized columns of A*V; with rank3 == false the third is the cross product of the
// first two, which is what a rank-2 matrix (an essential matrix) leaves defined.  A is destroyed.
HS_HD inline void jacobi_svd3(double* A, double* U, double* w, double* Vt, bool rank3) {
  double V[9], n2[3];
  jacobi_cols<3, 3>(A, V);
  jacobi_min_col<3, 3>(A, n2);
  int o[3] = {0, 1, 2};
  for (int i = 1; i < 3; i++)  // insertion sort, descending, stable
    for (int j = i; j > 0 && n2[o[j]] > n2[o[j - 1]]; j--) {
      const int x = o[j];
      o[j] = o[j - 1];
      o[j - 1] = x;
    }
  for (int k = 0; k < 3; k++) {
    w[k] = sqrt(n2[o[k]]);
    for (int i = 0; i < 3; i++) Vt[k * 3 + i] = V[i * 3 + o[k]];
  }
  for (int k = 0; k < 3; k++)
    for (int i = 0; i < 3; i++) U[i * 3 + k] = A[i * 3 + o[k]] / w[k];
  if (rank3) return;
  U[0 * 3 + 2] = U[1 * 3 + 0] * U[2 * 3 + 1] - U[2 * 3 + 0] * U[1 * 3 + 1];
  U[1 * 3 + 2] = U[2 * 3 + 0] * U[0 * 3 + 1] - U[0 * 3 + 0] * U[2 * 3 + 1];
  U[2 * 3 + 2] = U[0 * 3 + 0] * U[1 * 3 + 1] - U[1 * 3 + 0] * U[0 * 3 + 1];
}

HS_HD inline double det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// c = a * b, 3 x 3 row-major, every entry (a0*b0 + a1*b1) + a2*b2
HS_HD inline void mul3(const double* a, const double* b, double* c) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) c[i * 3 + j] = (a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j]) + a[i * 3 + 2] * b[6 + j];
}

// inverse by the adjugate: inv = adj / det
HS_HD inline void inv3(const double* m, double* o) {
  const double d = det3(m);
  o[0] = (m[4] * m[8] - m[5] * m[7]) / d;
  o[1] = (m[2] * m[7] - m[1] * m[8]) / d;
  o[2] = (m[1] * m[5] - m[2] * m[4]) / d;
  o[3] = (m[5] * m[6] - m[3] * m[8]) / d;
  o[4] = (m[0] * m[8] - m[2] * m[6]) / d;
  o[5] = (m[2] * m[3] - m[0] * m[5]) / d;
  o[6] = (m[3] * m[7] - m[4] * m[6]) / d;
  o[7] = (m[1] * m[6] - m[0] * m[7]) / d;
  o[8] = (m[0] * m[4] - m[1] * m[3]) / d;
}

}  // namespace hs
