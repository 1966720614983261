// twoview_main.cpp — h-slam_amd/csrc/hs_jacobi.h and hs_twoview_rule.h on the host: the very inlines the kernels of
// hs_twoview_kernels.hip call, driven from stdin by tests/test_twoview.py (built there with
// g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined).
//   twoview_main null   lines "M a_0 .. a_{M*9-1}" (M = 8 or 16, hex doubles, row-major M x 9)
//                       -> the 9 entries of hs::jacobi_null_vector as hex doubles, then the sweeps run
//   twoview_main null4  lines of 16 hex doubles (4 x 4) -> the 4 entries of the null vector
//   twoview_main svd3   lines "rank3 a_0 .. a_8" -> U (9), w (3), Vt (9) of hs::jacobi_svd3
//   twoview_main rule   lines "model N g_0 .. g_7 p_0 .. p_7" (p: float bit patterns in hex) -> "ok why best"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../h-slam_amd/csrc/hs_jacobi.h"
#include "../../h-slam_amd/csrc/hs_twoview_rule.h"

static double hexd(const std::string& s) { return std::strtod(s.c_str(), nullptr); }

static float bitsf(const std::string& s) {
  const unsigned u = (unsigned)std::strtoul(s.c_str(), nullptr, 16);
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

template <int M>
static void null_of(const std::vector<double>& in) {
  double A[M * 9], V[81], n2[9];
  for (int i = 0; i < M * 9; i++) A[i] = in[i];
  const int sweeps = hs::jacobi_cols<M, 9>(A, V);
  const int j = hs::jacobi_min_col<M, 9>(A, n2);
  for (int i = 0; i < 9; i++) std::printf("%a ", V[i * 9 + j]);
  std::printf("%d\n", sweeps);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string mode = argv[1];
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::vector<std::string> tok;
    for (std::string t; is >> t;) tok.push_back(t);
    if (tok.empty()) continue;
    if (mode == "null") {
      const int M = std::atoi(tok[0].c_str());
      if ((M != 8 && M != 16) || (int)tok.size() != 1 + M * 9) return 3;
      std::vector<double> in;
      for (size_t i = 1; i < tok.size(); i++) in.push_back(hexd(tok[i]));
      if (M == 8) null_of<8>(in);
      else null_of<16>(in);
    } else if (mode == "null4") {
      if (tok.size() != 16) return 3;
      double A[16], v[4];
      for (int i = 0; i < 16; i++) A[i] = hexd(tok[i]);
      hs::jacobi_null_vector<4, 4>(A, v);
      std::printf("%a %a %a %a\n", v[0], v[1], v[2], v[3]);
    } else if (mode == "svd3") {
      if (tok.size() != 10) return 3;
      double A[9], U[9], w[3], Vt[9];
      for (int i = 0; i < 9; i++) A[i] = hexd(tok[1 + i]);
      hs::jacobi_svd3(A, U, w, Vt, std::atoi(tok[0].c_str()) != 0);
      for (int i = 0; i < 9; i++) std::printf("%a ", U[i]);
      for (int i = 0; i < 3; i++) std::printf("%a ", w[i]);
      for (int i = 0; i < 9; i++) std::printf("%a ", Vt[i]);
      std::printf("\n");
    } else if (mode == "rule") {
      if (tok.size() != 18) return 3;
      const int model = std::atoi(tok[0].c_str()), N = std::atoi(tok[1].c_str());
      int g[8];
      float p[8];
      for (int i = 0; i < 8; i++) {
        g[i] = std::atoi(tok[2 + i].c_str());
        p[i] = bitsf(tok[10 + i]);
      }
      const hs::TwoViewPick r = model ? hs::twoview_rule_f(g, p, N, 1.0f, 50) : hs::twoview_rule_h(g, p, N, 1.0f, 50);
      std::printf("%d %d %d\n", r.ok, r.why, r.best);
    } else {
      return 2;
    }
  }
  return 0;
}
