// hs_frame_rule.h — System::flagFramesForMarginalization (Src/FullSystemMarginalize.cpp:18-103), written once for
// the device kernel (hs_k_win_flag_frames, hs_map_kernels.hip) and the host (hs_debug_frame_rule, the CPU test of the
// rule).  The reference's types are kept: the float comparison in < minPointsRemaining * (in + out), the float
// fabs(logf((float)refToFh[0])), the double distScore and the sqrtf on the pair (frame -> newest).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/hs_map.h"
#include "hs_layout.h"

#ifndef HS_HD
#define HS_HD __host__ __device__
#endif

namespace hs {

// the clauses a frame's flag came from (hs_debug_frame_rule's why[]; the kernel does not keep them)
enum {
  HS_FRAME_WHY_POINTS = 1,   // in < minPointsRemaining * (in + out)
  HS_FRAME_WHY_AFFINE = 2,   // |log(affine factor)| > maxLogAffFacInWindow
  HS_FRAME_WHY_SCORE = 4,    // the smallest distance score
  HS_FRAME_WHY_AGE = 8,      // the minFrameAge > maxFrames branch
  HS_FRAME_WHY_BLOCKED = 16  // a clause held, but size - flagged had reached minFrames
};

// nF window frames (window order, the newest last).  in / out: the frames' point counts; aff0: refToFh[0] of
// AffLight::fromToVecExposure(newest, frame); dist: distanceLL of the pair (host h, target t) at [h * nF + t], a float
// as FrameFramePrecalc keeps it; kf_id: KfId.  flagged[nF] is written (1 = flagged by this call), why[nF] (nullable)
// the clauses.  Returns the number of flagged frames.
HS_HD inline int frame_rule(int nF, const int* in, const int* out, const double* aff0, const float* dist,
                            const int* kf_id, const hs_frame_marg_params& P, uint8_t* flagged, uint8_t* why) {
  for (int f = 0; f < nF; f++) {
    flagged[f] = 0;
    if (why) why[f] = 0;
  }
  if (nF <= 0) return 0;
  int n = 0;
  if (P.minFrameAge > P.maxFrames) {
    for (int i = P.maxFrames; i < nF; i++) {
      if (i - P.maxFrames < 0) continue;  // a negative maxFrames would index before the window
      if (!flagged[i - P.maxFrames]) n++;
      flagged[i - P.maxFrames] = 1;
      if (why) why[i - P.maxFrames] |= HS_FRAME_WHY_AGE;
    }
    return n;
  }
  // marginalize all frames that have not enough points or too different a brightness
  for (int f = 0; f < nF; f++) {
    const bool few = (float)in[f] < P.minPointsRemaining * (float)(in[f] + out[f]);
    const bool aff = fabsf(logf((float)aff0[f])) > P.maxLogAffFacInWindow;
    if (!(few || aff)) continue;
    if (nF - n > P.minFrames) {
      flagged[f] = 1;
      n++;
      if (why) why[f] |= (few ? HS_FRAME_WHY_POINTS : 0) | (aff ? HS_FRAME_WHY_AFFINE : 0);
    } else if (why) {
      why[f] |= HS_FRAME_WHY_BLOCKED;
    }
  }
  // marginalize one
  if (nF - n >= P.maxFrames) {
    double smallest = 1;
    int pick = -1;
    const int latest = kf_id[nF - 1];
    for (int f = 0; f < nF; f++) {
      if (kf_id[f] > latest - P.minFrameAge || kf_id[f] == 0) continue;
      double score = 0;
      for (int t = 0; t < nF; t++) {
        if (kf_id[t] > latest - P.minFrameAge + 1 || t == f) continue;
        score += 1 / (1e-5 + dist[f * nF + t]);
      }
      score *= -sqrtf(dist[f * nF + nF - 1]);
      if (score < smallest) {
        smallest = score;
        pick = f;
      }
    }
    // no candidate: the reference dereferences an empty toMarginalize here; nothing more is flagged
    if (pick >= 0) {
      if (!flagged[pick]) n++;
      flagged[pick] = 1;
      if (why) why[pick] |= HS_FRAME_WHY_SCORE;
    }
  }
  return n;
}

}  // namespace hs
