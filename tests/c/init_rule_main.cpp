// Stand-alone host run of h-slam_amd/csrc/hs_init_rule.h, the decision hs_k_init_seed makes per key
// (System::InitFromInitializer, Src/System.cpp:265-290).  tests/test_init_rule.py compiles this file with the host
// compiler alone (no HIP) and feeds it the cases:
//   g++ -std=c++17 -O1 -ffp-contract=off tests/c/init_rule_main.cpp -o init_rule_main
// stdin, one case per line:  tri good idepth invz colours_finite x y W H   (floats as the hex of their 32 bits)
// stdout, one line per case: videpth (hex of its bits) and the code
#include <cstdint>
#include <cstdio>
#include <cstring>

#define HS_HD
#include "../../h-slam_amd/csrc/hs_init_rule.h"

static float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

int main() {
  int tri, good, fin, W, H;
  uint32_t id, iz, x, y;
  while (std::scanf("%d %d %x %x %d %x %x %d %d", &tri, &good, &id, &iz, &fin, &x, &y, &W, &H) == 9) {
    const float vid = hs::init_videpth(tri != 0, good != 0, from_bits(id), from_bits(iz));
    const int code = hs::init_rule(vid, fin != 0, from_bits(x), from_bits(y), W, H);
    uint32_t vb;
    std::memcpy(&vb, &vid, 4);
    std::printf("%08x %d\n", vb, code);
  }
  return 0;
}
