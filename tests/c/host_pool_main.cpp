// Stand-alone host check of h-slam_amd/csrc/hs_host.h's allocation owner on a machine without a HIP device, where
// every HIP allocation fails: a failed allocation reports HS_ERR_HIP, leaves its slot null and the process-wide live
// count at 0, and releasing what was never allocated is harmless.  Linked against libhslam_amd.so (hs_last_error, the
// live count); tests/test_host_pool.py builds and runs it.  Under host sanitizers, by hand:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include tests/c/host_pool_main.cpp -o host_pool_main \
//       -Lh-slam_amd/lib -lhslam_amd -Wl,-rpath,$PWD/h-slam_amd/lib -L/opt/rocm/lib -lamdhip64
#include <cstdio>
#include <cstring>

#include "../../h-slam_amd/csrc/hs_host.h"
#include "../../include/hs_ba.h"

extern "C" long long hs_debug_live_allocations(void);

static int bad = 0;
#define CHECK(x)                                          \
  do {                                                    \
    if (!(x)) {                                           \
      std::printf("line %d: %s does not hold\n", __LINE__, #x); \
      bad++;                                              \
    }                                                     \
  } while (0)

static bool have_error() { return std::strlen(hs_last_error()) > 0; }
static void clear_error() { hs::g_err.clear(); }

struct Object {  // the shape of every object behind the ABI: slots owned by a pool
  hs::Pool pool;
  float* d_a = nullptr;
  double* d_b = nullptr;
  int* h_c = nullptr;
};

int main() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
    std::printf("a HIP device is visible: allocations succeed, nothing to check here\n");
    return 0;
  }
  CHECK(hs::check_device(0) == HS_ERR_HIP);
  CHECK(have_error());
  CHECK(hs_debug_live_allocations() == 0);

  Object* o = new Object();
  clear_error();
  CHECK(o->pool.alloc(&o->d_a, 1024) == HS_ERR_HIP);
  CHECK(o->d_a == nullptr && have_error());
  clear_error();
  CHECK(o->pool.alloc_zero(&o->d_b, 16, nullptr) == HS_ERR_HIP);
  CHECK(o->d_b == nullptr && have_error());
  clear_error();
  CHECK(o->pool.pinned(&o->h_c, 8) == HS_ERR_HIP);
  CHECK(o->h_c == nullptr && have_error());
  clear_error();
  CHECK(o->pool.pinned(&o->h_c, 8, hipHostMallocMapped | hipHostMallocCoherent) == HS_ERR_HIP);
  CHECK(o->h_c == nullptr && have_error());
  CHECK(hs_debug_live_allocations() == 0);

  o->pool.release(&o->d_a);  // a null slot, never recorded
  o->pool.release(&o->h_c);
  CHECK(o->d_a == nullptr && o->h_c == nullptr);
  o->pool.release_all();  // an empty pool
  o->pool.release_all();
  CHECK(hs_debug_live_allocations() == 0);
  delete o;

  {  // a one-shot entry point's scratch: the pool leaves scope after a failed allocation
    hs::Pool scratch;
    float* d_tmp = nullptr;
    CHECK(scratch.alloc_zero(&d_tmp, 0, nullptr) == HS_ERR_HIP);  // n = 0 asks for one element
    CHECK(d_tmp == nullptr);
  }
  CHECK(hs_debug_live_allocations() == 0);

  hs::Device dev;  // open fails before it creates anything; close on the unopened rest is harmless
  CHECK(dev.open(0) == HS_ERR_HIP);
  CHECK(dev.stream == nullptr && dev.e0 == nullptr && dev.e1 == nullptr);
  dev.close();

  std::printf("%d checks failed\n", bad);
  return bad ? 1 : 0;
}
