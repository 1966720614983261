// hs_extract.cpp — the extractor context of include/hs_extract.h: argument checks, the blur weights and umax by
// their rules on the host, and one extract as a chain of launches on the extractor's stream that ends in the single
// 4-byte read of the key count.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/hs_ba.h"
#include "../../include/hs_extract.h"
#include "hs_extract_kernels.h"
#include "../../include/hs_image.h"
#include "hs_host.h"
#include "hs_image_kernels.h"
#include "hs_sel_kernels.h"
#include "hs_undist_kernels.h"

// one extract's outputs; two sets, so that an extract that overflows leaves the previous result untouched
struct hs_extract_result {
  float *x = nullptr, *y = nullptr, *angle = nullptr;
  uint32_t* desc = nullptr;
  uint8_t* blurred = nullptr;
};

struct hs_extractor : hs::Device {
  hs::Pool pool;
  int W = 0, H = 0, cap = 0;
  int alloc = 0;  // min(cap, interior size): entries of the per-key arrays
  hipEvent_t e_consumed = nullptr;  // a consumer's reads of the key arrays (hs_extract_keys_consumed)
  bool consumer_pending = false;
  int w[4] = {0, 0, 0, 0};
  unsigned long long umax = 0;
  float* d_map = nullptr;    // the caller's map (hs_extractor_extract)
  uint8_t* d_img = nullptr;  // cvImgL
  bool have_img = false;     // an extract has filled d_img (hs_extract_image)
  char4* d_pattern = nullptr;
  int* d_row_cnt = nullptr;
  int* d_count = nullptr;
  int* h_count = nullptr;  // pinned
  hs_extract_result res[2];
  int cur = 0;  // res[cur] is the last successful extract
  int n = 0;
  float last_ms = 0;
};

namespace {

// Gaussian taps for sigma 2 as 8-bit fixed point: the normalised kernel in double times 256, rounded from the outer
// tap inward with the rounding error carried into the next tap; the centre takes what is left of 256
void blur_weights(int w[4]) {
  double g[7], sum = 0;
  for (int k = 0; k < 7; k++) sum += g[k] = std::exp(-(k - 3) * (k - 3) / (2.0 * 2.0 * 2.0));
  double err = 0;
  int others = 0;
  for (int k = 0; k < 3; k++) {
    const double v = g[k] / sum * 256.0 + err;
    w[k] = (int)std::nearbyint(v);
    err = v - w[k];
    others += 2 * w[k];
  }
  w[3] = 256 - others;
}

// InitUmax's rule for half patch 15: the disc's half width per row, rounded for the rows up to 45 degrees and
// mirrored about the diagonal for the rest; packed 4 bits per row
unsigned long long make_umax() {
  const int hp = kExtHalfPatch;
  int um[kExtHalfPatch + 2] = {0};
  const int vmax = (int)std::floor(hp * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil(hp * std::sqrt(2.f) / 2);
  for (int v = 0; v <= vmax; v++) um[v] = (int)std::nearbyint(std::sqrt((double)hp * hp - v * v));
  for (int v = hp, v0 = 0; v >= vmin; --v) {
    while (um[v0] == um[v0 + 1]) ++v0;
    um[v] = v0;
    ++v0;
  }
  unsigned long long p = 0;
  for (int v = 0; v <= hp; v++) p |= (unsigned long long)(um[v] & 15) << (4 * v);
  return p;
}

// everything after the inputs are on the device (or enqueued on e->stream): the kernels into the spare result set,
// the count's read, the swap.  d_map_src: the map to scan (the extractor's own or the selector's).
int run_extract(hs_extractor* e, const float* d_map_src, hs_undistorter* u, const uint8_t* raw, int* n_keys) {
  hs_extract_result& r = e->res[e->cur ^ 1];
  hipStream_t s = e->stream;
  HS_HIP(hipEventRecord(e->e0, s));
  if (u) HS_HIP(hs_undist_enqueue(u, s, raw, nullptr, e->d_img));
  HsExtBlurArgs b;
  b.W = e->W;
  b.H = e->H;
  for (int k = 0; k < 4; k++) b.w[k] = e->w[k];
  b.src = e->d_img;
  b.dst = r.blurred;
  hipLaunchKernelGGL(hs_k_ext_blur, dim3((e->W + kExtBlurTileW - 1) / kExtBlurTileW, (e->H + kExtBlurTileH - 1) / kExtBlurTileH),
                     dim3(256), 0, s, b);
  HS_HIP(hipGetLastError());
  HsExtKeysArgs k;
  k.W = e->W;
  k.H = e->H;
  k.cap = e->alloc;  // == cap unless cap exceeds the interior, which no count can
  k.map = d_map_src;
  k.row_cnt = e->d_row_cnt;
  k.x = r.x;
  k.y = r.y;
  k.count = e->d_count;
  const int rows = e->H - 2 * kExtBorder;
  hipLaunchKernelGGL(hs_k_ext_count, dim3((rows + 3) / 4), dim3(256), 0, s, k);
  HS_HIP(hipGetLastError());
  hipLaunchKernelGGL(hs_k_ext_write, dim3((rows + 3) / 4), dim3(256), 0, s, k);
  HS_HIP(hipGetLastError());
  HsExtDescArgs d;
  d.W = e->W;
  d.cap = k.cap;
  d.umax = e->umax;
  d.count = e->d_count;
  d.x = r.x;
  d.y = r.y;
  d.img = e->d_img;
  d.blurred = r.blurred;
  d.pattern = e->d_pattern;
  d.angle = r.angle;
  d.desc = r.desc;
  // a wave per key over a grid that does not depend on the count: the count is read on the device
  hipLaunchKernelGGL(hs_k_ext_desc, dim3(std::min((k.cap + 3) / 4, 2048)), dim3(256), 0, s, d);
  HS_HIP(hipGetLastError());
  HS_HIP(hipEventRecord(e->e1, s));
  HS_HIP(hipMemcpyAsync(e->h_count, e->d_count, sizeof(int), hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));  // the one wait of an extract
  e->have_img = true;
  HS_HIP(hipEventElapsedTime(&e->last_ms, e->e0, e->e1));
  const int n = *e->h_count;
  if (n_keys) *n_keys = n;
  if (n > e->cap)
    return hs::fail(HS_ERR_INVALID, "extract yields " + std::to_string(n) + " keys, capacity is " + std::to_string(e->cap));
  e->cur ^= 1;
  e->n = n;
  return HS_OK;
}

// A consumer (hs_tracer_add_keys) may still be reading the current result set on its own stream.  This extract
// writes the other set and only the one after it reuses the set being read, but ordering the very next extract
// behind the consumer's reads costs nothing and needs no bookkeeping per set.
int begin_extract(hs_extractor* e) {
  HS_HIP(hipSetDevice(e->device));
  if (e->consumer_pending) {
    HS_HIP(hipStreamWaitEvent(e->stream, e->e_consumed, 0));
    e->consumer_pending = false;
  }
  return HS_OK;
}

}  // namespace

void hs_extract_keys(hs_extractor* e, int* device, int* W, int* H, int* n, const float** d_x, const float** d_y,
                     hipEvent_t* ready) {
  *device = e->device;
  *W = e->W;
  *H = e->H;
  *n = e->n;
  *d_x = e->res[e->cur].x;
  *d_y = e->res[e->cur].y;
  *ready = e->e1;
}

bool hs_extract_image(hs_extractor* e, int* device, int* W, int* H, const uint8_t** d_img, hipEvent_t* ready) {
  *device = e->device;
  *W = e->W;
  *H = e->H;
  *d_img = e->d_img;
  *ready = e->e1;
  return e->have_img;
}

hipError_t hs_extract_keys_consumed(hs_extractor* e, hipStream_t consumer) {
  const hipError_t rc = hipEventRecord(e->e_consumed, consumer);
  if (rc == hipSuccess) e->consumer_pending = true;
  return rc;
}

extern "C" {

int hs_extractor_create(hs_extractor** out, int device_id, int width, int height, int capacity,
                        const int8_t pattern[1024]) {
  if (!out) return hs::fail(HS_ERR_INVALID, "null out");
  *out = nullptr;
  if (!pattern) return hs::fail(HS_ERR_INVALID, "null pattern");
  if (width < 2 * kExtBorder + 1 || height < 2 * kExtBorder + 1)
    return hs::fail(HS_ERR_INVALID, "image smaller than 39 x 39: no pixel lies 19 px from every edge");
  if ((long long)width * height >= (1LL << 30)) return hs::fail(HS_ERR_INVALID, "image too large");
  if (capacity < 1) return hs::fail(HS_ERR_INVALID, "capacity must be >= 1");
  for (int i = 0; i < 1024; i++)
    if (pattern[i] < -kExtPatternMax || pattern[i] > kExtPatternMax)
      return hs::fail(HS_ERR_INVALID, "pattern entry " + std::to_string(i) + " outside +-13: a rotated tap could leave the image");
  HS_TRY(hs::check_device(device_id));
  hs_extractor* e = new hs_extractor();
  e->W = width;
  e->H = height;
  e->cap = capacity;
  const long long interior = (long long)(width - 2 * kExtBorder) * (height - 2 * kExtBorder);
  e->alloc = (int)std::min<long long>(capacity, interior);
  blur_weights(e->w);
  e->umax = make_umax();
  const size_t area = (size_t)width * height, c = e->alloc;
  int rc = [&]() -> int {
    hs::Pool& m = e->pool;
    HS_TRY(e->open(device_id));
    HS_HIP(hipEventCreateWithFlags(&e->e_consumed, hipEventDisableTiming));
    HS_TRY(m.alloc(&e->d_map, area));
    HS_TRY(m.alloc(&e->d_img, area));
    HS_TRY(m.alloc(&e->d_pattern, 256));
    HS_TRY(m.alloc(&e->d_row_cnt, height - 2 * kExtBorder));
    HS_TRY(m.alloc(&e->d_count, 1));
    HS_TRY(m.pinned(&e->h_count, 1));
    for (hs_extract_result& r : e->res) {
      HS_TRY(m.alloc(&r.x, c));
      HS_TRY(m.alloc(&r.y, c));
      HS_TRY(m.alloc(&r.angle, c));
      HS_TRY(m.alloc(&r.desc, c * 8));
      HS_TRY(m.alloc(&r.blurred, area));
      // fills on the kernels' own stream (hs_extractor_get before any extract reads blurred)
      HS_HIP(hipMemsetAsync(r.blurred, 0, area, e->stream));
    }
    HS_HIP(hipMemsetAsync(e->d_count, 0, sizeof(int), e->stream));
    HS_HIP(hipMemcpyAsync(e->d_pattern, pattern, 1024, hipMemcpyHostToDevice, e->stream));
    HS_HIP(hipStreamSynchronize(e->stream));  // pattern is the caller's
    return HS_OK;
  }();
  if (rc) hs_extractor_destroy(e);
  else *out = e;
  return rc;
}

void hs_extractor_destroy(hs_extractor* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->consumer_pending) (void)hipEventSynchronize(e->e_consumed);  // a tracer may still be copying the keys
  e->pool.release_all();
  if (e->e_consumed) (void)hipEventDestroy(e->e_consumed);
  e->close();
  delete e;
}

int hs_extractor_extract(hs_extractor* e, const float* map, const uint8_t* img8, int* n_keys) {
  if (!e || !map || !img8) return hs::fail(HS_ERR_INVALID, "null argument");
  HS_TRY(begin_extract(e));
  const size_t area = (size_t)e->W * e->H;
  HS_HIP(hipMemcpyAsync(e->d_map, map, area * sizeof(float), hipMemcpyHostToDevice, e->stream));
  HS_HIP(hipMemcpyAsync(e->d_img, img8, area, hipMemcpyHostToDevice, e->stream));
  return run_extract(e, e->d_map, nullptr, nullptr, n_keys);
}

int hs_extractor_extract_selected(hs_extractor* e, hs_selector* s, const uint8_t* img8, int* n_keys) {
  if (!e || !s || !img8) return hs::fail(HS_ERR_INVALID, "null argument");
  const float* d_map = nullptr;
  hipEvent_t ready = nullptr;
  HS_TRY(hs_select_device_map(s, e->device, e->W, e->H, &d_map, &ready));
  HS_TRY(begin_extract(e));
  HS_HIP(hipStreamWaitEvent(e->stream, ready, 0));
  HS_HIP(hipMemcpyAsync(e->d_img, img8, (size_t)e->W * e->H, hipMemcpyHostToDevice, e->stream));
  return run_extract(e, d_map, nullptr, nullptr, n_keys);
}

int hs_extractor_extract_u8(hs_extractor* e, hs_selector* s, hs_undistorter* u, const uint8_t* raw, int* n_keys) {
  if (!e || !s || !u || !raw) return hs::fail(HS_ERR_INVALID, "null argument");
  HS_TRY(hs_undist_match(u, e->device, e->W, e->H));
  const float* d_map = nullptr;
  hipEvent_t ready = nullptr;
  HS_TRY(hs_select_device_map(s, e->device, e->W, e->H, &d_map, &ready));
  HS_TRY(begin_extract(e));
  HS_HIP(hipStreamWaitEvent(e->stream, ready, 0));
  return run_extract(e, d_map, u, raw, n_keys);
}

// The same, with cvImgL copied device to device from a device image (include/hs_image.h) behind its last set.
int hs_extractor_extract_image(hs_extractor* e, hs_selector* s, hs_image* im, int* n_keys) {
  if (!e || !s || !im) return hs::fail(HS_ERR_INVALID, "null argument");
  HsImageView v;
  HS_TRY(hs_image_view(im, e->device, e->W, e->H, 1, true, &v));
  const float* d_map = nullptr;
  hipEvent_t ready = nullptr;
  HS_TRY(hs_select_device_map(s, e->device, e->W, e->H, &d_map, &ready));
  HS_TRY(begin_extract(e));
  HS_HIP(hipStreamWaitEvent(e->stream, ready, 0));
  HS_HIP(hipStreamWaitEvent(e->stream, v.ready, 0));
  HS_HIP(hipMemcpyAsync(e->d_img, v.img8, (size_t)e->W * e->H, hipMemcpyDeviceToDevice, e->stream));
  HS_HIP(hs_image_consumed(im, e->stream));
  return run_extract(e, d_map, nullptr, nullptr, n_keys);
}

int hs_extractor_get(hs_extractor* e, int* n, float* xy, float* angle, uint8_t* desc, uint8_t* blurred) {
  if (!e) return hs::fail(HS_ERR_INVALID, "null extractor");
  HS_HIP(hipSetDevice(e->device));
  const hs_extract_result& r = e->res[e->cur];
  const size_t m = e->n;
  if (n) *n = e->n;
  std::vector<float> hx(xy ? m : 0), hy(xy ? m : 0);
  hipStream_t s = e->stream;
  if (xy && m) {
    HS_HIP(hipMemcpyAsync(hx.data(), r.x, m * sizeof(float), hipMemcpyDeviceToHost, s));
    HS_HIP(hipMemcpyAsync(hy.data(), r.y, m * sizeof(float), hipMemcpyDeviceToHost, s));
  }
  if (angle && m) HS_HIP(hipMemcpyAsync(angle, r.angle, m * sizeof(float), hipMemcpyDeviceToHost, s));
  if (desc && m) HS_HIP(hipMemcpyAsync(desc, r.desc, m * 32, hipMemcpyDeviceToHost, s));
  if (blurred) HS_HIP(hipMemcpyAsync(blurred, r.blurred, (size_t)e->W * e->H, hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  for (size_t i = 0; i < hx.size(); i++) {
    xy[2 * i] = hx[i];
    xy[2 * i + 1] = hy[i];
  }
  return HS_OK;
}

int hs_extractor_last_stats(hs_extractor* e, double* ms) {
  if (!e) return hs::fail(HS_ERR_INVALID, "null extractor");
  if (ms) *ms = e->last_ms;
  return HS_OK;
}

}  // extern "C"
