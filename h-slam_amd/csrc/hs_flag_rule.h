// hs_flag_rule.h — System::flagPointsForRemoval's per-point decision (Src/Mapping.cpp:248-328) with
// MapPoint::isOOB / isInlierNew (Include/MapPoint.h:133-161), written once for the device kernel (hs_k_win_flag,
// hs_win_kernels.hip) and the host (hs_debug_flag_rule, the CPU test of the rule).
#pragma once
#include "../../include/hs_types.h"

#ifndef HS_HD
#define HS_HD __host__ __device__
#endif

namespace hs {

constexpr int kMinGoodActiveResForMarg = 3;  // setting_minGoodActiveResForMarg (Src/Settings.cpp:96)
constexpr int kMinGoodResForMarg = 4;        // setting_minGoodResForMarg (:97)
constexpr double kMinIdepthHMarg = 50.0;     // setting_minIdepthH_marg (:119)

// the result of flag_rule: the action in bits 0-1, the reference's counters this point adds to above them
enum {
  HS_FLAG_KEEP = 0, HS_FLAG_DROP = 1, HS_FLAG_MARG = 2, HS_FLAG_ACTION = 3,
  HS_FLAG_NORES = 4,  // flag_nores: idepth < 0 or no residual
  HS_FLAG_OOB = 8,    // flag_oob: isOOB or the host is marginalized
  HS_FLAG_IN = 16,    // flag_in: ... and isInlierNew
  HS_FLAG_ININ = 32   // flag_inin: ... and idepth_hessian > setting_minIdepthH_marg
};

// nres: residual-list length; vis: its residuals in state IN into a frame that is marginalized; nGood:
// numGoodResiduals; hdif: the last solve's HdiF (idepth_hessian = 1 / HdiF, compared in fp64); last0 / last1:
// lastResiduals[0 / 1].second; host_flagged: the host frame is marginalized.
HS_HD inline int flag_rule(int nres, int vis, int nGood, float idepth, float hdif, int last0, int last1,
                           bool host_flagged) {
  if (idepth < 0 || nres == 0) return HS_FLAG_DROP | HS_FLAG_NORES;
  bool oob = nres >= kMinGoodActiveResForMarg && nGood > kMinGoodResForMarg + 10 &&
             nres - vis < kMinGoodActiveResForMarg;
  oob = oob || last0 == HS_RES_OOB;
  oob = oob || (nres >= 2 && last0 == HS_RES_OUT && last1 == HS_RES_OUT);
  if (!(oob || host_flagged)) return HS_FLAG_KEEP;
  if (!(nres >= kMinGoodActiveResForMarg && nGood >= kMinGoodResForMarg)) return HS_FLAG_DROP | HS_FLAG_OOB;
  if (hdif > 0 && 1.0 / (double)hdif > kMinIdepthHMarg) return HS_FLAG_MARG | HS_FLAG_OOB | HS_FLAG_IN | HS_FLAG_ININ;
  return HS_FLAG_DROP | HS_FLAG_OOB | HS_FLAG_IN;
}

}  // namespace hs
