// hs_host.h — what every host translation unit behind the C ABI starts from (private to the library): the error
// plumbing of hs_last_error(), the device check and the stream + timing events of one object, and the owner of its
// device and pinned memory.  A new ABI row takes its errors, device, stream and memory from here.
// HS_HOST_ERRORS_ONLY before the include leaves the HIP half out (hs_undist_tables.cpp: plain C++, no HIP types).
#pragma once
#include <string>

#include "../../include/hs_types.h"

namespace hs {
extern thread_local std::string g_err;  // hs_last_error(), shared by every entry point of the library
inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
}  // namespace hs

#define HS_TRY(x)        \
  do {                   \
    int rc_ = (x);       \
    if (rc_) return rc_; \
  } while (0)

#ifndef HS_HOST_ERRORS_ONLY
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <vector>

#define HS_HIP(x)                                                                                          \
  do {                                                                                                     \
    hipError_t e_ = (x);                                                                                   \
    if (e_ != hipSuccess) return hs::fail(HS_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));     \
  } while (0)

namespace hs {

// a create function's device check, before it allocates anything
inline int check_device(int device_id) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(HS_ERR_HIP, "no HIP device");
  if (device_id < 0 || device_id >= ndev) return fail(HS_ERR_INVALID, "bad device id");
  return HS_OK;
}

// the device an object lives on, the stream everything of it is enqueued on and its two timing events
struct Device {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int open(int device_id) {
    device = device_id;
    HS_HIP(hipSetDevice(device_id));
    HS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HS_HIP(hipEventCreate(&e0));
    HS_HIP(hipEventCreate(&e1));
    return HS_OK;
  }
  void close() {  // after the owner's pools are released
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (stream) (void)hipStreamDestroy(stream);
    e0 = e1 = nullptr;
    stream = nullptr;
  }
};

extern std::atomic<long long> g_live;  // allocations handed out by every Pool and not yet freed (hs_ba.cpp)

// Owner of device and pinned allocations.  It records the slot (the pointer variable), not the value: release nulls
// the slot, and two recorded slots may swap their values (the HdiF ping-pong) and are still freed once each.  A slot
// must outlive its pool's release and must not move; pointers into an allocation are not recorded.  Regrowing is
// release, then alloc (alloc on a recorded slot releases it first).  A local Pool owns the scratch of a one-shot entry point: every return path frees it.
class Pool {
 public:
  Pool() = default;
  Pool(const Pool&) = delete;
  Pool& operator=(const Pool&) = delete;
  ~Pool() { release_all(); }

  template <typename T>
  int alloc(T** p, size_t n) {
    return get((void**)p, n * sizeof(T), false, 0);
  }
  // Allocate and zero-fill n elements; the fill is enqueued on `s`, the stream every later user of the buffer runs
  // on.  (A null-stream hipMemset returns before the fill lands and does not order against a hipStreamNonBlocking
  // stream: an object's first kernel could store into a buffer that the fill then zeroed --
  // tools/micro/memset_order.hip.)
  template <typename T>
  int alloc_zero(T** p, size_t n, hipStream_t s) {
    if (n == 0) n = 1;
    HS_TRY(alloc(p, n));
    HS_HIP(hipMemsetAsync(*p, 0, n * sizeof(T), s));
    return HS_OK;
  }
  template <typename T>
  int pinned(T** p, size_t n, unsigned flags = hipHostMallocDefault) {
    return get((void**)p, n * sizeof(T), true, flags);
  }
  template <typename T>
  void release(T** p) {
    for (size_t i = 0; i < recs_.size(); i++)
      if (recs_[i].slot == (void**)p) {
        drop(recs_[i]);
        recs_.erase(recs_.begin() + i);
        return;
      }
  }
  void release_all() {
    for (const Rec& r : recs_) drop(r);
    recs_.clear();
  }

 private:
  struct Rec {
    void** slot;
    bool pinned;
  };
  std::vector<Rec> recs_;

  int get(void** slot, size_t bytes, bool pin, unsigned flags) {
    release(slot);  // a slot filled before (a retry after a failure half-way) is not lost
    *slot = nullptr;
    const hipError_t e = pin ? hipHostMalloc(slot, bytes, flags) : hipMalloc(slot, bytes);
    if (e != hipSuccess) {
      *slot = nullptr;
      return fail(HS_ERR_HIP, std::string(pin ? "hipHostMalloc" : "hipMalloc") + " of " + std::to_string(bytes) +
                                  " bytes: " + hipGetErrorString(e));
    }
    if (*slot) {
      recs_.push_back({slot, pin});
      g_live.fetch_add(1, std::memory_order_relaxed);
    }
    return HS_OK;
  }
  static void drop(const Rec& r) {
    if (!*r.slot) return;
    (void)(r.pinned ? hipHostFree(*r.slot) : hipFree(*r.slot));
    *r.slot = nullptr;
    g_live.fetch_sub(1, std::memory_order_relaxed);
  }
};

// (I, dx, dy) triplets as the float4 texels the kernels read
inline void texels_from_triplets(float4* dst, const float* src, size_t n) {
  for (size_t i = 0; i < n; i++) dst[i] = make_float4(src[3 * i], src[3 * i + 1], src[3 * i + 2], 0.f);
}

}  // namespace hs
#endif  // HS_HOST_ERRORS_ONLY
