// hs_twoview_rule.h — the two decisions that end Initializer::ReconstructF (Src/Initializer.cpp:840-913) and
// Initializer::ReconstructH (:1032-1072), written once for the device kernel (hs_k_tv_finish,
// hs_twoview_kernels.hip) and the host (tests/c/twoview_main.cpp, the CPU test of the rule).
#pragma once

#ifndef HS_HD
#ifdef __HIPCC__
#define HS_HD __host__ __device__
#else
#define HS_HD
#endif
#endif

namespace hs {

// hs_twoview_result.why
enum {
  HS_TV_OK = 0,
  HS_TV_NO_SCORE = 1,     // no hypothesis scored above 0
  HS_TV_H_SINGULAR = 2,   // d1 / d2 or d2 / d3 < 1.00001 (:941)
  HS_TV_NO_WINNER = 3,    // no clear winner among the motion hypotheses, or too few good points
  HS_TV_LOW_PARALLAX = 4  // the winner's parallax is below minParallax
};

struct TwoViewPick {
  int ok, why, best;  // best: the motion hypothesis that won (-1: none)
};

// ReconstructF.  nGood / parallax: CheckRT's results for (R1, t), (R2, t), (R1, -t), (R2, -t); N: the inliers of F.
HS_HD inline TwoViewPick twoview_rule_f(const int* nGood, const float* parallax, int N, float minParallax,
                                        int minTriangulated) {
  TwoViewPick r = {0, HS_TV_NO_WINNER, -1};
  int maxGood = nGood[0];                                        // :840
  for (int i = 1; i < 4; i++)
    if (nGood[i] > maxGood) maxGood = nGood[i];
  const int n09 = static_cast<int>(0.9 * N);                     // :845
  const int nMinGood = n09 > minTriangulated ? n09 : minTriangulated;
  int nsimilar = 0;                                              // :847-855
  for (int i = 0; i < 4; i++)
    if (nGood[i] > 0.7 * maxGood) nsimilar++;
  if (maxGood < nMinGood || nsimilar > 1) return r;              // :858
  // :864-911: an else-if chain, so only the first hypothesis that attains maxGood is looked at
  for (int i = 0; i < 4; i++)
    if (maxGood == nGood[i]) {
      r.best = i;
      if (parallax[i] > minParallax) {
        r.ok = 1;
        r.why = HS_TV_OK;
      } else {
        r.why = HS_TV_LOW_PARALLAX;
      }
      return r;
    }
  return r;
}

// ReconstructH.  nGood / parallax: CheckRT's results for the 8 hypotheses of Faugeras' method; N: the inliers of H.
HS_HD inline TwoViewPick twoview_rule_h(const int* nGood, const float* parallax, int N, float minParallax,
                                        int minTriangulated) {
  int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;   // :1032-1035
  float bestParallax = -1;
  for (int i = 0; i < 8; i++) {                                 // :1041-1060
    if (nGood[i] > bestGood) {
      secondBestGood = bestGood;
      bestGood = nGood[i];
      bestSolutionIdx = i;
      bestParallax = parallax[i];
    } else if (nGood[i] > secondBestGood) {
      secondBestGood = nGood[i];
    }
  }
  TwoViewPick r = {0, HS_TV_NO_WINNER, bestSolutionIdx};
  const bool counts = secondBestGood < 0.75 * bestGood && bestGood > minTriangulated && bestGood > 0.9 * N;  // :1062
  if (!counts) return r;
  if (bestParallax >= minParallax) {
    r.ok = 1;
    r.why = HS_TV_OK;
  } else {
    r.why = HS_TV_LOW_PARALLAX;
  }
  return r;
}

}  // namespace hs
