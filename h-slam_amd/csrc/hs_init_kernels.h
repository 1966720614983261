// hs_init_kernels.h — argument blocks of the initializer hand-off kernels (hs_init_kernels.hip, include/hs_init.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hs_refine_kernels.h"
#include "hs_win_kernels.h"

// DirectRefinement's Pnt set-up (Src/Initializer.cpp:1362-1382) from keys that lie on the device: every plane
// hs_refiner_set_points uploads, with the same values
struct HsRefPointsArgs {
  int n, W, H;
  int n_planes;          // float planes of the refiner's state block, n floats each
  int pl_u, pl_v, pl_invz, pl_id, pl_idn, pl_ir;  // the planes that are not zero
  const float2* first;   // FirstFramePts = mvKeys[i].pt
  const uint8_t* tri;    // Triangulated[i]
  const float* z;        // Pts3D[i].z
  float* pf;             // [n_planes][n]
  uint8_t* pb;           // tri | good | good_new, n bytes each
  int* n_bad;            // += keys outside hs_refiner_set_points' range (zero on entry)
};

// System::InitFromInitializer's point loop (Src/System.cpp:265-290): one workgroup, stable compaction of the seeded
// keys into HsStagedPoint records
struct HsInitSeedArgs {
  int n, W, H;
  int base;              // first free entry of `out`
  int room;              // entries of `out` from `base` on: a record past it is counted and not written
  const float4* img;     // the first frame, level 0
  const float* u;
  const float* v;
  const float* invz;
  const float* idepth;
  const uint8_t* tri;
  const uint8_t* good;
  float outlierTHSumComponent;
  float priorF;          // setting_idepthFixPrior * SCALE_IDEPTH^2 (hasDepthPrior)
  uint8_t* why;          // [n] hs_init_rule.h's code per key
  int* n_seeded;
  HsStagedPoint* out;
};

__global__ void hs_k_ref_points(HsRefPointsArgs a);
__global__ void hs_k_init_seed(HsInitSeedArgs a);
