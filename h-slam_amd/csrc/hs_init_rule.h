// hs_init_rule.h — System::InitFromInitializer's per-key decision (Src/System.cpp:265-290) and the videpth array it
// reads (Src/Initializer.cpp:155-159, then DirectRefinement's write-back at :1393-1397), written once for the device
// kernel (hs_k_init_seed, hs_init_kernels.hip) and the host (hs_refiner_get_videpth; tests/c/init_rule_main.cpp, the CPU
// test of the rule).
#pragma once

#ifndef HS_HD
#define HS_HD __host__ __device__
#endif

namespace hs {

// why a key of the first frame did or did not become a point of the first window
enum {
  HS_INIT_SEEDED = 0,
  HS_INIT_NODEPTH = 1,    // videpth <= 0: not triangulated, or a depth that is not positive
  HS_INIT_NONFINITE = 2,  // energyTH not finite: one of the constructor's 8 colours is not finite
  HS_INIT_BORDER = 3      // the constructor's pattern would leave the image (hs_tracer_add_points' border rule)
};

// videpth[i]: -1 where the key was not triangulated; else 1 / Pts3D.z (invz), overwritten by the refined idepth where
// the point is still good.  Before a refine idepth == invz and good == 1: the constructor's array.
HS_HD inline float init_videpth(bool tri, bool good, float idepth, float invz) {
  return !tri ? -1.0f : (good ? idepth : invz);
}

// (x, y) = mvKeys[i].pt + 0.5f.  The reference builds the ImmaturePoint wherever the key lies and reads outside its
// image near the border; here such a key is skipped before the constructor runs (a documented deviation), so the
// border test comes before the colours are looked at.  A NaN videpth is not <= 0: it goes on, as in the reference.
HS_HD inline int init_rule(float videpth, bool colours_finite, float x, float y, int W, int H) {
  if (videpth <= 0.0f) return HS_INIT_NODEPTH;
  if (!(x >= 2 && y >= 2 && x < W - 3 && y < H - 3)) return HS_INIT_BORDER;
  if (!colours_finite) return HS_INIT_NONFINITE;
  return HS_INIT_SEEDED;
}

}  // namespace hs
