// hs_extract.cpp — the extractor context of include/hs_extract.h: argument checks, the blur weights and umax by
// their rules on the host, and one extract as a chain of launches on the extractor's stream that ends in the single
// 4-byte read of the key count.  The keys come from the selection map (run_extract) or from the corner detector
// (run_fast, hs_fast_kernels.hip); the blur, the descriptors and the closing read are shared.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/hs_ba.h"
#include "../../include/hs_extract.h"
#include "hs_extract_kernels.h"
#include "hs_fast_kernels.h"
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
  // the UseFAST branch (allocated by the first fast extract): mvKeys[i].response, the corners before Ssc in sorted
  // order, and {corners, width taken, corners taken}
  float* response = nullptr;
  int* s_idx = nullptr;
  uint8_t* s_resp = nullptr;
  int* info = nullptr;
  bool fast = false;  // this set holds a fast extract
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
  // scratch of the UseFAST branch, allocated by the first fast extract
  bool have_fast = false;
  int max_corners = 0;  // strict 3x3 maxima of a W x H plane with a 3-px band: no two are 8-neighbours
  uint8_t *d_resp = nullptr, *d_cresp = nullptr, *d_covered = nullptr, *d_occ = nullptr;
  int *d_frow_cnt = nullptr, *d_cidx = nullptr;
  int max_high = 0;  // Ssc evaluates the widths 1 .. max_high of a search, each in its own workgroup
  int *d_wtaken = nullptr, *d_wcnt = nullptr;
  size_t *d_woff = nullptr, *d_toff = nullptr;
  std::vector<size_t> h_toff;
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

// the launches both branches share: cvImgL's blur into the result set ...
int launch_blur(hs_extractor* e, hs_extract_result& r) {
  hipStream_t s = e->stream;
  HsExtBlurArgs b;
  b.W = e->W;
  b.H = e->H;
  for (int k = 0; k < 4; k++) b.w[k] = e->w[k];
  b.src = e->d_img;
  b.dst = r.blurred;
  hipLaunchKernelGGL(hs_k_ext_blur, dim3((e->W + kExtBlurTileW - 1) / kExtBlurTileW, (e->H + kExtBlurTileH - 1) / kExtBlurTileH),
                     dim3(256), 0, s, b);
  HS_HIP(hipGetLastError());
  return HS_OK;
}

// angle and descriptor of the keys that lie in r.x / r.y, their count in d_count
int launch_desc(hs_extractor* e, hs_extract_result& r) {
  HsExtDescArgs d;
  d.W = e->W;
  d.cap = e->alloc;
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
  hipLaunchKernelGGL(hs_k_ext_desc, dim3(std::min((d.cap + 3) / 4, 2048)), dim3(256), 0, e->stream, d);
  HS_HIP(hipGetLastError());
  return HS_OK;
}

// the closing event, the count's read and the one wait; on success the spare set becomes the result
int finish_extract(hs_extractor* e, int* n_keys, bool fast) {
  hipStream_t s = e->stream;
  HS_HIP(hipEventRecord(e->e1, s));
  HS_HIP(hipMemcpyAsync(e->h_count, e->d_count, sizeof(int), hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));  // the one wait of an extract
  e->have_img = true;
  HS_HIP(hipEventElapsedTime(&e->last_ms, e->e0, e->e1));
  const int n = *e->h_count;
  if (n_keys) *n_keys = n;
  if (n > e->cap)
    return hs::fail(HS_ERR_INVALID, "extract yields " + std::to_string(n) + " keys, capacity is " + std::to_string(e->cap));
  // (n <= alloc = min(cap, interior) here.  A fast extract's keys may lie on x = W-19 / y = H-19, outside the
  // interior, but they are strict 3x3 maxima: at most ceil((W-37)/2) * ceil((H-37)/2) <= (W-38) * (H-38) of them.)
  e->cur ^= 1;
  e->n = n;
  e->res[e->cur].fast = fast;
  return HS_OK;
}

// everything after the inputs are on the device (or enqueued on e->stream): the kernels into the spare result set,
// the count's read, the swap.  d_map_src: the map to scan (the extractor's own or the selector's).
int run_extract(hs_extractor* e, const float* d_map_src, hs_undistorter* u, const uint8_t* raw, int* n_keys) {
  hs_extract_result& r = e->res[e->cur ^ 1];
  hipStream_t s = e->stream;
  HS_HIP(hipEventRecord(e->e0, s));
  if (u) HS_HIP(hs_undist_enqueue(u, s, raw, nullptr, e->d_img));
  HS_TRY(launch_blur(e, r));
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
  HS_TRY(launch_desc(e, r));
  return finish_extract(e, n_keys, false);
}

// ---- the UseFAST branch

int check_fast_params(const hs_fast_params* p) {
  if (!p) return hs::fail(HS_ERR_INVALID, "null params");
  if (p->threshold < 0 || p->threshold > 254) return hs::fail(HS_ERR_INVALID, "threshold must lie in [0, 254]");
  if (p->num_features < 2) return hs::fail(HS_ERR_INVALID, "num_features must be >= 2");
  if (p->min_dist < 0) return hs::fail(HS_ERR_INVALID, "min_dist must be >= 0");
  if (!(p->tolerance >= 0.f && p->tolerance < 1.f)) return hs::fail(HS_ERR_INVALID, "tolerance must lie in [0, 1)");
  return HS_OK;
}

// the detector's buffers, on the first fast extract: an extractor that never detects pays nothing
// A retry after a failure half-way allocates again from the start; hs::Pool::alloc on a slot it already holds
// releases that allocation first, so nothing is held twice.
int ensure_fast(hs_extractor* e) {
  if (e->have_fast) return HS_OK;
  hs::Pool& m = e->pool;
  const int W = e->W, H = e->H;
  const size_t area = (size_t)W * H;
  e->max_corners = ((W - 2 * kFastRing + 1) / 2) * ((H - 2 * kFastRing + 1) / 2);
  const size_t mc = e->max_corners;
  // Ssc's widths.  The bracket's `high` falls as K grows, so its value at K = 2 bounds every search: one workgroup,
  // one covered grid and one taken list per width up to it.  Corners taken at one width have cells that differ by
  // 3 or more in a row or a column, so a grid of R x C cells takes at most ceil(R/3) * ceil(C/3) of them.
  const double exp1 = H + W + 4.0;
  const double exp2 = 4.0 * W + 8.0 + 8.0 * H + (double)H * H + (double)W * W - 2.0 * H * W + 8.0 * H * W;
  e->max_high = std::max(1, (int)-std::round(exp1 - std::sqrt(exp2)));
  std::vector<size_t> woff(e->max_high), toff(e->max_high);
  size_t cov = 0, tak = 0;
  for (int w = 1; w <= e->max_high; w++) {
    const size_t R = 2 * H / w + 1, C = 2 * W / w + 1;
    woff[w - 1] = cov;
    toff[w - 1] = tak;
    cov += (R * C + 15) / 16 * 16;
    tak += std::min(mc, ((R + 2) / 3) * ((C + 2) / 3));
  }
  HS_TRY(m.alloc(&e->d_resp, area));
  HS_TRY(m.alloc(&e->d_occ, area));
  HS_TRY(m.alloc(&e->d_covered, cov));
  HS_TRY(m.alloc(&e->d_wtaken, tak));
  HS_TRY(m.alloc(&e->d_wcnt, e->max_high));
  HS_TRY(m.alloc(&e->d_woff, e->max_high));
  HS_TRY(m.alloc(&e->d_toff, e->max_high));
  HS_TRY(m.alloc(&e->d_frow_cnt, H - 2 * kFastRing));
  HS_TRY(m.alloc(&e->d_cidx, mc));
  HS_TRY(m.alloc(&e->d_cresp, mc));
  for (hs_extract_result& r : e->res) {
    HS_TRY(m.alloc(&r.response, e->alloc));
    HS_TRY(m.alloc(&r.s_idx, mc));
    HS_TRY(m.alloc(&r.s_resp, mc));
    HS_TRY(m.alloc(&r.info, kFastInfoSize));
  }
  const size_t tb = sizeof(size_t) * e->max_high;
  HS_HIP(hipMemcpyAsync(e->d_woff, woff.data(), tb, hipMemcpyHostToDevice, e->stream));
  HS_HIP(hipMemcpyAsync(e->d_toff, toff.data(), tb, hipMemcpyHostToDevice, e->stream));
  HS_HIP(hipStreamSynchronize(e->stream));  // the tables are locals
  e->h_toff = toff;
  e->have_fast = true;
  return HS_OK;
}

// as run_extract, the keys coming from the detector; cvImgL is on the device or enqueued on e->stream (u: made here)
int run_fast(hs_extractor* e, const hs_fast_params* p, hs_undistorter* u, const uint8_t* raw, int* n_keys) {
  hs_extract_result& r = e->res[e->cur ^ 1];
  hipStream_t s = e->stream;
  HS_HIP(hipEventRecord(e->e0, s));
  if (u) HS_HIP(hs_undist_enqueue(u, s, raw, nullptr, e->d_img));
  HsFastArgs a;
  a.W = e->W;
  a.H = e->H;
  a.threshold = p->threshold;
  a.num_features = p->num_features;
  a.min_dist = std::min(p->min_dist, std::max(e->W, e->H));  // beyond the image's larger side nothing changes
  a.cap = e->alloc;
  a.tolerance = p->tolerance;
  a.img = e->d_img;
  a.resp = e->d_resp;
  a.row_cnt = e->d_frow_cnt;
  a.c_idx = e->d_cidx;
  a.c_resp = e->d_cresp;
  a.s_idx = r.s_idx;
  a.s_resp = r.s_resp;
  a.max_high = e->max_high;
  a.woff = e->d_woff;
  a.toff = e->d_toff;
  a.covered = e->d_covered;
  a.wtaken = e->d_wtaken;
  a.wcnt = e->d_wcnt;
  a.occ = e->d_occ;
  a.info = r.info;
  a.x = r.x;
  a.y = r.y;
  a.response = r.response;
  a.count = e->d_count;
  const int rows = e->H - 2 * kFastRing;
  HS_HIP(hipMemsetAsync(e->d_occ, 0, (size_t)e->W * e->H, s));
  hipLaunchKernelGGL(hs_k_fast_resp, dim3((e->W + kFastTileW - 1) / kFastTileW, (e->H + kFastTileH - 1) / kFastTileH),
                     dim3(256), 0, s, a);
  HS_HIP(hipGetLastError());
  hipLaunchKernelGGL(hs_k_fast_count, dim3((rows + 3) / 4), dim3(256), 0, s, a);
  HS_HIP(hipGetLastError());
  hipLaunchKernelGGL(hs_k_fast_write, dim3((rows + 3) / 4), dim3(256), 0, s, a);
  HS_HIP(hipGetLastError());
  hipLaunchKernelGGL(hs_k_fast_sort, dim3(1), dim3(256), 0, s, a);
  HS_HIP(hipGetLastError());
  hipLaunchKernelGGL(hs_k_fast_ssc, dim3(e->max_high), dim3(64), 0, s, a);
  HS_HIP(hipGetLastError());
  hipLaunchKernelGGL(hs_k_fast_final, dim3(1), dim3(64), 0, s, a);
  HS_HIP(hipGetLastError());
  HS_TRY(launch_blur(e, r));
  HS_TRY(launch_desc(e, r));
  return finish_extract(e, n_keys, true);
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

void hs_fast_params_default(hs_fast_params* p) {
  if (!p) return;
  p->threshold = 8;       // minThFAST
  p->num_features = 3000; // IndNumFeatures
  p->min_dist = 5;        // EnforcedMinDist
  p->tolerance = 0.1f;
}

int hs_extractor_extract_fast(hs_extractor* e, const hs_fast_params* p, const uint8_t* img8, int* n_keys) {
  if (!e || !img8) return hs::fail(HS_ERR_INVALID, "null argument");
  HS_TRY(check_fast_params(p));
  HS_TRY(begin_extract(e));
  HS_TRY(ensure_fast(e));
  HS_HIP(hipMemcpyAsync(e->d_img, img8, (size_t)e->W * e->H, hipMemcpyHostToDevice, e->stream));
  return run_fast(e, p, nullptr, nullptr, n_keys);
}

int hs_extractor_extract_fast_u8(hs_extractor* e, const hs_fast_params* p, hs_undistorter* u, const uint8_t* raw,
                                 int* n_keys) {
  if (!e || !u || !raw) return hs::fail(HS_ERR_INVALID, "null argument");
  HS_TRY(check_fast_params(p));
  HS_TRY(hs_undist_match(u, e->device, e->W, e->H));
  HS_TRY(begin_extract(e));
  HS_TRY(ensure_fast(e));
  return run_fast(e, p, u, raw, n_keys);
}

int hs_extractor_extract_fast_image(hs_extractor* e, const hs_fast_params* p, hs_image* im, int* n_keys) {
  if (!e || !im) return hs::fail(HS_ERR_INVALID, "null argument");
  HS_TRY(check_fast_params(p));
  HsImageView v;
  HS_TRY(hs_image_view(im, e->device, e->W, e->H, 1, true, &v));
  HS_TRY(begin_extract(e));
  HS_TRY(ensure_fast(e));
  HS_HIP(hipStreamWaitEvent(e->stream, v.ready, 0));
  HS_HIP(hipMemcpyAsync(e->d_img, v.img8, (size_t)e->W * e->H, hipMemcpyDeviceToDevice, e->stream));
  HS_HIP(hs_image_consumed(im, e->stream));
  return run_fast(e, p, nullptr, nullptr, n_keys);
}

int hs_extractor_get_fast(hs_extractor* e, int* n_corners, int* width, float* response, float* corner_xy,
                          float* corner_response) {
  if (!e) return hs::fail(HS_ERR_INVALID, "null extractor");
  const hs_extract_result& r = e->res[e->cur];
  if (!r.fast) return hs::fail(HS_ERR_STATE, "the current result is not a fast extract");
  HS_HIP(hipSetDevice(e->device));
  hipStream_t s = e->stream;
  int info[kFastInfoSize] = {0};
  HS_HIP(hipMemcpyAsync(info, r.info, sizeof(info), hipMemcpyDeviceToHost, s));
  if (response && e->n) HS_HIP(hipMemcpyAsync(response, r.response, (size_t)e->n * sizeof(float), hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  const size_t nc = info[kFastInfoCorners];
  if (n_corners) *n_corners = (int)nc;
  if (width) *width = info[kFastInfoWidth];
  if ((corner_xy || corner_response) && nc) {
    std::vector<int> idx(nc);
    std::vector<uint8_t> resp(nc);
    HS_HIP(hipMemcpyAsync(idx.data(), r.s_idx, nc * sizeof(int), hipMemcpyDeviceToHost, s));
    HS_HIP(hipMemcpyAsync(resp.data(), r.s_resp, nc, hipMemcpyDeviceToHost, s));
    HS_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < nc; i++) {
      if (corner_xy) {
        corner_xy[2 * i] = (float)(idx[i] % e->W);
        corner_xy[2 * i + 1] = (float)(idx[i] / e->W);
      }
      if (corner_response) corner_response[i] = (float)resp[i];
    }
  }
  return HS_OK;
}

// Test hook (not in the header): Ssc's bracket of the current fast result and what hs_k_fast_ssc left for width w,
// valid until the next fast extract call.  *count = -1 for a width outside [low, high]: no workgroup evaluated it.
// taken (nullable): the first min(*count, taken_cap) sorted indices that width took.
int hs_debug_fast_width(hs_extractor* e, int w, int* low, int* high, int* count, int* taken, int taken_cap) {
  if (!e || !low || !high || !count) return hs::fail(HS_ERR_INVALID, "null argument");
  const hs_extract_result& r = e->res[e->cur];
  if (!r.fast) return hs::fail(HS_ERR_STATE, "the current result is not a fast extract");
  HS_HIP(hipSetDevice(e->device));
  int info[kFastInfoSize] = {0};
  HS_HIP(hipMemcpy(info, r.info, sizeof(info), hipMemcpyDeviceToHost));
  *low = info[kFastInfoLow];
  *high = info[kFastInfoHigh];
  *count = -1;
  if (w < *low || w > *high || w < 1 || w > e->max_high) return HS_OK;
  HS_HIP(hipMemcpy(count, e->d_wcnt + (w - 1), sizeof(int), hipMemcpyDeviceToHost));
  const int m = std::min(*count, taken_cap);
  if (taken && m > 0)
    HS_HIP(hipMemcpy(taken, e->d_wtaken + e->h_toff[w - 1], sizeof(int) * m, hipMemcpyDeviceToHost));
  return HS_OK;
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
