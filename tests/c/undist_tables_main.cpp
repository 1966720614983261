// Stand-alone host check of h-slam_amd/csrc/hs_undist_tables.cpp (no HIP, no device): builds the remap tables of
// four calibrations and the photometric tables, and prints a checksum of each.  Meant to be compiled together with
// hs_undist_tables.cpp under host sanitizers and run by hand:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       tests/c/undist_tables_main.cpp h-slam_amd/csrc/hs_undist_tables.cpp -o undist_tables_main
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/hs_undist.h"

namespace hs {
thread_local std::string g_err;  // the library defines this next to hs_last_error; here the program stands alone
}

static hs_undist_calib calib(int model, int w_in, int h_in, int w_out, int h_out, int process, const double K[4],
                             const double dist[4], const double desK[4]) {
  hs_undist_calib c{};
  c.model = model;
  c.w_in = w_in;
  c.h_in = h_in;
  c.w_out = w_out;
  c.h_out = h_out;
  c.process = process;
  for (int i = 0; i < 4; i++) {
    c.K_in[i] = K[i];
    c.dist[i] = dist ? dist[i] : 0.0;
    c.desired_K[i] = desK ? desK[i] : 0.0;
  }
  return c;
}

static int run(const char* name, const hs_undist_calib& c) {
  const size_t n = (size_t)c.w_out * c.h_out;
  std::vector<float> rx(n), ry(n);
  float K[4];
  const int rc = hs_undist_make_remap(&c, K, rx.data(), ry.data());
  if (rc) {
    std::printf("%s: rc %d (%s)\n", name, rc, hs::g_err.c_str());
    return 1;
  }
  double sum = 0;
  size_t invalid = 0;
  for (size_t i = 0; i < n; i++) {
    sum += rx[i] + ry[i];
    invalid += rx[i] == -1;
  }
  std::printf("%s: K %.9g %.9g %.9g %.9g, sum %.9g, invalid %zu of %zu\n", name, K[0], K[1], K[2], K[3], sum, invalid, n);
  return 0;
}

int main() {
  const double euroc_dist[4] = {-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05};
  const double kitti_K[4] = {7.18856e+02, 7.18856e+02, 6.071928e+02, 1.852157e+02};
  const double euroc_K[4] = {458.654, 457.296, 367.215, 248.375};
  const double euroc_des[4] = {0.6, 0.9, 0.5, 0.5};
  const double small_K[4] = {60.0, 60.0, 47.5, 31.5};
  const double small_des[4] = {0.45, 0.6, 0.5, 0.5};
  int bad = 0;
  bad += run("kitti pinhole crop", calib(HS_CAM_PINHOLE, 1241, 376, 1232, 368, HS_UNDIST_CROP, kitti_K, nullptr, nullptr));
  bad += run("euroc radtan useK", calib(HS_CAM_RADTAN, 752, 480, 640, 480, HS_UNDIST_USEK, euroc_K, euroc_dist, euroc_des));
  bad += run("small radtan crop", calib(HS_CAM_RADTAN, 96, 64, 64, 48, HS_UNDIST_CROP, small_K, euroc_dist, nullptr));
  bad += run("small radtan useK", calib(HS_CAM_RADTAN, 96, 64, 64, 48, HS_UNDIST_USEK, small_K, euroc_dist, small_des));

  float G[256], Binv[256], B[256];
  for (int i = 0; i < 256; i++) G[i] = 3.0f + 0.7f * (float)i + 0.001f * (float)(i * i);
  const int n_in = 96 * 64;
  std::vector<uint16_t> vig(n_in);
  for (int i = 0; i < n_in; i++) vig[i] = (uint16_t)(20000 + (i * 7919) % 45536);
  std::vector<float> vinv(n_in);
  int rc = hs_undist_make_photometric(G, vig.data(), n_in, Binv, B, vinv.data());
  double s = 0;
  for (int i = 0; i < 256; i++) s += Binv[i] + B[i];
  for (int i = 0; i < n_in; i++) s += vinv[i];
  std::printf("photometric: rc %d, sum %.9g\n", rc, s);
  bad += rc != 0;
  rc = hs_undist_make_photometric(nullptr, nullptr, 0, Binv, B, nullptr);
  std::printf("photometric identity: rc %d, B[200] %.9g\n", rc, B[200]);
  bad += rc != 0;
  G[100] = G[99];
  rc = hs_undist_make_photometric(G, nullptr, 0, Binv, B, nullptr);
  std::printf("photometric non-increasing G: rc %d (%s)\n", rc, hs::g_err.c_str());
  bad += rc != HS_ERR_INVALID;
  return bad ? 1 : 0;
}
