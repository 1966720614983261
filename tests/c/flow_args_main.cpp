// Stand-alone host check of h-slam_amd/csrc/hs_flow.cpp's argument validation: every path here returns before any
// device call, so it runs the same with and without a HIP device.  tests/test_flow.py compiles this file together with
// hs_flow.cpp under the host sanitizers and links the rest (hs_last_error, the kernels' host stubs) from
// libhslam_amd.so:
//   hipcc --cuda-host-only -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=all -x hip tests/c/flow_args_main.cpp h-slam_amd/csrc/hs_flow.cpp \
//       -o flow_args_main -Lh-slam_amd/lib -lhslam_amd -Wl,-rpath,$PWD/h-slam_amd/lib
#include <climits>
#include <cstdio>
#include <cstring>

#include "../../include/hs_ba.h"
#include "../../include/hs_flow.h"

static int bad = 0;
#define CHECK(x)                                                \
  do {                                                          \
    if (!(x)) {                                                 \
      std::printf("line %d: %s does not hold\n", __LINE__, #x); \
      bad++;                                                    \
    }                                                           \
  } while (0)

static bool error_says(const char* word) { return std::strstr(hs_last_error(), word) != nullptr; }

int main() {
  hs_flow* f = reinterpret_cast<hs_flow*>(0x1);  // must come back null from every failed create
  CHECK(hs_flow_create(nullptr, 0, 64, 48, 10) == HS_ERR_INVALID && error_says("null"));
  CHECK(hs_flow_create(&f, 0, 15, 48, 10) == HS_ERR_INVALID && f == nullptr && error_says("16"));
  f = reinterpret_cast<hs_flow*>(0x1);
  CHECK(hs_flow_create(&f, 0, 64, 15, 10) == HS_ERR_INVALID && f == nullptr);
  f = reinterpret_cast<hs_flow*>(0x1);
  CHECK(hs_flow_create(&f, 0, -5, INT_MIN, 10) == HS_ERR_INVALID && f == nullptr);
  f = reinterpret_cast<hs_flow*>(0x1);
  CHECK(hs_flow_create(&f, 0, 64, 48, 0) == HS_ERR_INVALID && f == nullptr && error_says("capacity"));
  f = reinterpret_cast<hs_flow*>(0x1);
  CHECK(hs_flow_create(&f, 0, 64, 48, INT_MIN) == HS_ERR_INVALID && f == nullptr);
  f = reinterpret_cast<hs_flow*>(0x1);
  CHECK(hs_flow_create(&f, 0, INT_MAX, INT_MAX, 10) == HS_ERR_INVALID && f == nullptr && error_says("large"));
  f = reinterpret_cast<hs_flow*>(0x1);
  CHECK(hs_flow_create(&f, 0, 1 << 15, 1 << 14, 10) == HS_ERR_INVALID && f == nullptr);  // 2^29 padded pixels and more

  // a null context, and null buffers in front of it, are refused before anything is read
  uint8_t img[4] = {0, 0, 0, 0};
  float xy[2] = {0.f, 0.f}, out[2] = {0.f, 0.f}, err = 0.f, mean = 0.f;
  uint8_t status = 0;
  int n = -7;
  double ms = 0;
  long long its = 0;
  hs_extractor* no_extractor = nullptr;
  hs_undistorter* no_undistorter = nullptr;
  hs_flow_destroy(nullptr);
  CHECK(hs_flow_set_first(nullptr, img, 1, xy) == HS_ERR_INVALID);
  CHECK(hs_flow_set_first_extracted(nullptr, no_extractor, &n) == HS_ERR_INVALID && n == -7);
  CHECK(hs_flow_track(nullptr, img, 7.f, &n) == HS_ERR_INVALID && n == -7);
  CHECK(hs_flow_track_extracted(nullptr, no_extractor, 7.f, &n) == HS_ERR_INVALID && n == -7);
  CHECK(hs_flow_track_u8(nullptr, no_undistorter, img, 7.f, &n) == HS_ERR_INVALID && n == -7);
  CHECK(hs_flow_get(nullptr, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == HS_ERR_INVALID && n == -7);
  CHECK(hs_flow_mean_flow(nullptr, &mean) == HS_ERR_INVALID && mean == 0.f);
  CHECK(hs_flow_calc(nullptr, img, img, 1, xy, nullptr, out, &status, &err) == HS_ERR_INVALID);
  CHECK(hs_flow_get_pyramid(nullptr, 0, 0, nullptr, nullptr, &n, &n) == HS_ERR_INVALID && n == -7);
  CHECK(hs_flow_last_stats(nullptr, &ms, &its, &n) == HS_ERR_INVALID && n == -7);
  CHECK(std::strlen(hs_last_error()) > 0);

  std::printf("%d checks failed\n", bad);
  return bad ? 1 : 0;
}
