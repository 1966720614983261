// hs_flow.cpp — the keypoint-flow context of include/hs_flow.h: argument checks, the frame slots (padded levels and
// derivatives) and FindMatches' bookkeeping around one launch of the tracker kernel per call.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/hs_ba.h"
#include "../../include/hs_flow.h"
#include "../../include/hs_image.h"
#include "hs_extract_kernels.h"
#include "hs_flow_kernels.h"
#include "hs_host.h"
#include "hs_image_kernels.h"
#include "hs_undist_kernels.h"

// one frame: every level's image with its reflected border, and its derivative with a zero border
struct hs_flow_slot {
  uint8_t* img = nullptr;
  short2* deriv = nullptr;
};

// counters of one call, written by the tracker kernel and read back with the call's one wait
struct hs_flow_counts {
  unsigned long long iters;
  int n_good;
  int pad;
};

struct hs_flow : hs::Device {
  hs::Pool pool;
  int W = 0, H = 0, cap = 0;
  HsFlowLevels lv;
  size_t slot_elems = 0;    // elements of one slot's image (and derivative) buffer
  hs_flow_slot slot[4];     // 0, 1: the tracked frames, swapping on every track; 2, 3: hs_flow_calc's pair
  int cur = 0;              // slot[cur] is TransitImage
  int last[2] = {-1, -1};   // the slots of the last calc / track: previous, next
  uint8_t* d_raw = nullptr;  // W*H: an uploaded or undistorted cvImgL before it is padded
  float2* d_first = nullptr;  // FirstFramePts
  float2* d_pts[2] = {nullptr, nullptr};  // d_pts[pcur] = MatchedPts (= mvbPrevMatched), d_pts[pcur ^ 1] = MatchedPtsBkp
  int pcur = 0;
  uint8_t *d_status = nullptr, *d_good = nullptr;
  float* d_err = nullptr;
  // hs_flow_calc's own points and outputs: the tracked state is not touched
  float2 *d_cprev = nullptr, *d_cinit = nullptr, *d_cxy = nullptr;
  uint8_t *d_cstatus = nullptr, *d_cgood = nullptr;
  float* d_cerr = nullptr;
  hs_flow_counts* d_counts = nullptr;
  hs_flow_counts* h_counts = nullptr;  // pinned
  float* d_mean = nullptr;             // hs_flow_mean_flow_device's result
  float* h_mean = nullptr;             // pinned
  int n = 0;
  bool have_first = false, tracked = false;
  long long first_id = 0;  // counts the first frames set
  float last_ms = 0;
  long long last_iters = 0;
};

namespace {

// buildOpticalFlowPyramid's stop rule: level l+1 exists while l < 2 and both halved sizes exceed the window
void make_levels(int w, int h, HsFlowLevels* lv, size_t* elems) {
  lv->n = 0;
  size_t off = 0;
  for (int l = 0; l < kFlowMaxLevels; l++) {
    if (l > 0) {
      w = (w + 1) / 2;
      h = (h + 1) / 2;
      if (w <= kFlowWin || h <= kFlowWin) break;
    }
    lv->w[l] = w;
    lv->h[l] = h;
    lv->off[l] = (int)off;
    off += (size_t)(w + 2 * kFlowPad) * (h + 2 * kFlowPad);
    lv->n = l + 1;
  }
  for (int l = lv->n; l < kFlowMaxLevels; l++) lv->w[l] = lv->h[l] = lv->off[l] = 0;
  *elems = off;
}

inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }

// enqueues slot k's levels and derivatives from the plain W x H image at d_src
int build_slot(hs_flow* f, int k, const uint8_t* d_src) {
  const HsFlowLevels& lv = f->lv;
  hs_flow_slot& s = f->slot[k];
  hipStream_t st = f->stream;
  for (int l = 0; l < lv.n; l++) {
    const size_t padded = (size_t)(lv.w[l] + 2 * kFlowPad) * (lv.h[l] + 2 * kFlowPad);
    if (l == 0) {
      HsFlowPadArgs p;
      p.w = lv.w[0];
      p.h = lv.h[0];
      p.src = d_src;
      p.dst = s.img;
      hipLaunchKernelGGL(hs_k_flow_pad, dim3(blocks(padded)), dim3(256), 0, st, p);
    } else {
      HsFlowDownArgs d;
      d.sw = lv.w[l - 1];
      d.sh = lv.h[l - 1];
      d.dw = lv.w[l];
      d.dh = lv.h[l];
      d.src = s.img + lv.off[l - 1];
      d.dst = s.img + lv.off[l];
      hipLaunchKernelGGL(hs_k_flow_pyrdown, dim3(blocks(padded)), dim3(256), 0, st, d);
    }
    HS_HIP(hipGetLastError());
    HsFlowScharrArgs c;
    c.w = lv.w[l];
    c.h = lv.h[l];
    c.img = s.img + lv.off[l];
    c.deriv = s.deriv + lv.off[l];
    hipLaunchKernelGGL(hs_k_flow_scharr, dim3(blocks(padded)), dim3(256), 0, st, c);
    HS_HIP(hipGetLastError());
  }
  return HS_OK;
}

struct LkIo {
  const float2 *prev_xy, *init_xy;
  float2* xy;
  uint8_t *status, *good;
  float* err;
};

// enqueues the counters' reset and the tracker over n points from slot `sp` to slot `sn`
int enqueue_lk(hs_flow* f, int sp, int sn, int n, const LkIo& io, float max_l1_error) {
  HS_HIP(hipMemsetAsync(f->d_counts, 0, sizeof(hs_flow_counts), f->stream));
  if (n == 0) return HS_OK;
  HsFlowLkArgs a;
  a.lv = f->lv;
  a.prev_img = f->slot[sp].img;
  a.prev_deriv = f->slot[sp].deriv;
  a.next_img = f->slot[sn].img;
  a.n = n;
  a.prev_xy = io.prev_xy;
  a.init_xy = io.init_xy;
  a.xy = io.xy;
  a.status = io.status;
  a.err = io.err;
  a.good = io.good;
  a.max_l1_error = max_l1_error;
  a.n_good = &f->d_counts->n_good;
  a.n_iters = &f->d_counts->iters;
  hipLaunchKernelGGL(hs_k_flow_lk, dim3((n + 3) / 4), dim3(256), 0, f->stream, a);
  HS_HIP(hipGetLastError());
  return HS_OK;
}

// the end of a calc / track: the closing event, the counters' read and the call's one wait
int finish(hs_flow* f) {
  HS_HIP(hipEventRecord(f->e1, f->stream));
  HS_HIP(hipMemcpyAsync(f->h_counts, f->d_counts, sizeof(hs_flow_counts), hipMemcpyDeviceToHost, f->stream));
  HS_HIP(hipStreamSynchronize(f->stream));
  HS_HIP(hipEventElapsedTime(&f->last_ms, f->e0, f->e1));
  f->last_iters = (long long)f->h_counts->iters;
  return HS_OK;
}

// one FindMatches once the new frame's plain image is at d_src (or enqueued to be): build the spare slot, track the
// current points into the spare point buffer, swap both
int run_track(hs_flow* f, const uint8_t* d_src, float max_l1_error, int* n_good) {
  const int sp = f->cur, sn = f->cur ^ 1;
  HS_TRY(build_slot(f, sn, d_src));
  LkIo io;
  io.prev_xy = f->d_pts[f->pcur];
  io.init_xy = f->d_pts[f->pcur];  // USE_INITIAL_FLOW with the same vector; without the flag the start is the same
  io.xy = f->d_pts[f->pcur ^ 1];
  io.status = f->d_status;
  io.good = f->d_good;
  io.err = f->d_err;
  HS_TRY(enqueue_lk(f, sp, sn, f->n, io, max_l1_error));
  HS_TRY(finish(f));
  f->cur = sn;
  f->pcur ^= 1;
  f->last[0] = sp;
  f->last[1] = sn;
  f->tracked = true;
  if (n_good) *n_good = f->h_counts->n_good;
  return HS_OK;
}

// the first frame once its image is at d_src and its points are in d_first (both enqueued)
int finish_first(hs_flow* f, const uint8_t* d_src, int n) {
  hipStream_t s = f->stream;
  HS_TRY(build_slot(f, f->cur, d_src));
  if (n) {
    HS_HIP(hipMemcpyAsync(f->d_pts[0], f->d_first, (size_t)n * sizeof(float2), hipMemcpyDeviceToDevice, s));
    HS_HIP(hipMemcpyAsync(f->d_pts[1], f->d_first, (size_t)n * sizeof(float2), hipMemcpyDeviceToDevice, s));
    HS_HIP(hipMemsetAsync(f->d_status, 0, n, s));
    HS_HIP(hipMemsetAsync(f->d_good, 0, n, s));
    HS_HIP(hipMemsetAsync(f->d_err, 0, (size_t)n * sizeof(float), s));
  }
  HS_HIP(hipStreamSynchronize(s));
  f->n = n;
  f->have_first = true;
  f->tracked = false;
  f->first_id++;
  if (f->last[0] < 2) f->last[0] = f->last[1] = -1;  // a track's pair is gone; a calc's pair has slots of its own
  return HS_OK;
}

int extractor_image(hs_flow* f, hs_extractor* e, const uint8_t** d_img, hipEvent_t* ready) {
  int dev = 0, w = 0, h = 0;
  if (!hs_extract_image(e, &dev, &w, &h, d_img, ready))
    return hs::fail(HS_ERR_STATE, "the extractor has not extracted yet: it holds no image");
  if (dev != f->device) return hs::fail(HS_ERR_INVALID, "extractor and flow are on different devices");
  if (w != f->W || h != f->H) return hs::fail(HS_ERR_INVALID, "extractor size differs from the flow's");
  return HS_OK;
}

int need_first(const hs_flow* f) {
  if (!f->have_first) return hs::fail(HS_ERR_STATE, "no first frame: hs_flow_set_first comes before a track");
  return HS_OK;
}

}  // namespace

bool hs_flow_first_points(hs_flow* f, int* device, int* W, int* H, int* n, const float2** d_first) {
  *device = f->device;
  *W = f->W;
  *H = f->H;
  *n = f->n;
  *d_first = f->d_first;
  return f->have_first;
}

bool hs_flow_tracked_keys(hs_flow* f, HsFlowKeys* k) {
  k->device = f->device;
  k->n = f->n;
  k->first_id = f->first_id;
  k->tracked = f->tracked;
  k->first = f->d_first;
  k->matched = f->d_pts[f->pcur];
  k->good = f->d_good;
  k->stream = f->stream;
  return f->have_first;
}

extern "C" {

int hs_flow_create(hs_flow** out, int device_id, int width, int height, int capacity) {
  if (!out) return hs::fail(HS_ERR_INVALID, "null out");
  *out = nullptr;
  if (width < kFlowPad + 1 || height < kFlowPad + 1)
    return hs::fail(HS_ERR_INVALID, "image smaller than 16 x 16: a 15 px border cannot be reflected");
  if (((long long)width + 2 * kFlowPad) * ((long long)height + 2 * kFlowPad) >= (1LL << 29))
    return hs::fail(HS_ERR_INVALID, "image too large");
  if (capacity < 1) return hs::fail(HS_ERR_INVALID, "capacity must be >= 1");
  HS_TRY(hs::check_device(device_id));
  hs_flow* f = new hs_flow();
  f->W = width;
  f->H = height;
  f->cap = capacity;
  make_levels(width, height, &f->lv, &f->slot_elems);
  const size_t c = capacity;
  int rc = [&]() -> int {
    hs::Pool& m = f->pool;
    HS_TRY(f->open(device_id));
    for (hs_flow_slot& s : f->slot) {
      HS_TRY(m.alloc(&s.img, f->slot_elems));
      HS_TRY(m.alloc(&s.deriv, f->slot_elems));
      // hs_flow_get_pyramid may read a slot no call has filled
      HS_HIP(hipMemsetAsync(s.img, 0, f->slot_elems, f->stream));
      HS_HIP(hipMemsetAsync(s.deriv, 0, f->slot_elems * sizeof(short2), f->stream));
    }
    HS_TRY(m.alloc(&f->d_raw, (size_t)width * height));
    HS_TRY(m.alloc(&f->d_first, c));
    HS_TRY(m.alloc(&f->d_pts[0], c));
    HS_TRY(m.alloc(&f->d_pts[1], c));
    HS_TRY(m.alloc(&f->d_status, c));
    HS_TRY(m.alloc(&f->d_good, c));
    HS_TRY(m.alloc(&f->d_err, c));
    HS_TRY(m.alloc(&f->d_cprev, c));
    HS_TRY(m.alloc(&f->d_cinit, c));
    HS_TRY(m.alloc(&f->d_cxy, c));
    HS_TRY(m.alloc(&f->d_cstatus, c));
    HS_TRY(m.alloc(&f->d_cgood, c));
    HS_TRY(m.alloc(&f->d_cerr, c));
    HS_TRY(m.alloc(&f->d_counts, 1));
    HS_TRY(m.pinned(&f->h_counts, 1));
    HS_TRY(m.alloc(&f->d_mean, 1));
    HS_TRY(m.pinned(&f->h_mean, 1));
    HS_HIP(hipStreamSynchronize(f->stream));
    return HS_OK;
  }();
  if (rc) hs_flow_destroy(f);
  else *out = f;
  return rc;
}

void hs_flow_destroy(hs_flow* f) {
  if (!f) return;
  (void)hipSetDevice(f->device);
  if (f->stream) (void)hipStreamSynchronize(f->stream);
  f->pool.release_all();
  f->close();
  delete f;
}

int hs_flow_set_first(hs_flow* f, const uint8_t* img8, int n, const float* xy) {
  if (!f || !img8 || (n > 0 && !xy)) return hs::fail(HS_ERR_INVALID, "null argument");
  if (n < 0 || n > f->cap)
    return hs::fail(HS_ERR_INVALID, std::to_string(n) + " points, capacity is " + std::to_string(f->cap));
  HS_HIP(hipSetDevice(f->device));
  HS_HIP(hipMemcpyAsync(f->d_raw, img8, (size_t)f->W * f->H, hipMemcpyHostToDevice, f->stream));
  if (n) HS_HIP(hipMemcpyAsync(f->d_first, xy, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, f->stream));
  return finish_first(f, f->d_raw, n);
}

int hs_flow_set_first_extracted(hs_flow* f, hs_extractor* e, int* n_out) {
  if (!f || !e) return hs::fail(HS_ERR_INVALID, "null argument");
  const uint8_t* d_img = nullptr;
  hipEvent_t ready = nullptr;
  HS_TRY(extractor_image(f, e, &d_img, &ready));
  int dev = 0, w = 0, h = 0, n = 0;
  const float *d_x = nullptr, *d_y = nullptr;
  hs_extract_keys(e, &dev, &w, &h, &n, &d_x, &d_y, &ready);
  if (n > f->cap)
    return hs::fail(HS_ERR_INVALID, "extractor holds " + std::to_string(n) + " keys, capacity is " + std::to_string(f->cap));
  HS_HIP(hipSetDevice(f->device));
  HS_HIP(hipStreamWaitEvent(f->stream, ready, 0));
  if (n) {
    // the extractor keeps x and y apart
    hipLaunchKernelGGL(hs_k_flow_pack_xy, dim3(blocks(n)), dim3(256), 0, f->stream, n, d_x, d_y, f->d_first);
    HS_HIP(hipGetLastError());
  }
  HS_TRY(finish_first(f, d_img, n));  // waits: the extractor's buffers are free again when this returns
  if (n_out) *n_out = n;
  return HS_OK;
}

int hs_flow_track(hs_flow* f, const uint8_t* img8, float max_l1_error, int* n_good) {
  if (!f || !img8) return hs::fail(HS_ERR_INVALID, "null argument");
  HS_TRY(need_first(f));
  HS_HIP(hipSetDevice(f->device));
  HS_HIP(hipMemcpyAsync(f->d_raw, img8, (size_t)f->W * f->H, hipMemcpyHostToDevice, f->stream));
  HS_HIP(hipEventRecord(f->e0, f->stream));
  return run_track(f, f->d_raw, max_l1_error, n_good);
}

int hs_flow_track_extracted(hs_flow* f, hs_extractor* e, float max_l1_error, int* n_good) {
  if (!f || !e) return hs::fail(HS_ERR_INVALID, "null argument");
  const uint8_t* d_img = nullptr;
  hipEvent_t ready = nullptr;
  HS_TRY(extractor_image(f, e, &d_img, &ready));
  HS_TRY(need_first(f));
  HS_HIP(hipSetDevice(f->device));
  HS_HIP(hipStreamWaitEvent(f->stream, ready, 0));
  HS_HIP(hipEventRecord(f->e0, f->stream));
  return run_track(f, d_img, max_l1_error, n_good);  // waits: the extractor's image is free again on return
}

int hs_flow_track_u8(hs_flow* f, hs_undistorter* u, const uint8_t* raw, float max_l1_error, int* n_good) {
  if (!f || !u || !raw) return hs::fail(HS_ERR_INVALID, "null argument");
  HS_TRY(hs_undist_match(u, f->device, f->W, f->H));
  HS_TRY(need_first(f));
  HS_HIP(hipSetDevice(f->device));
  HS_HIP(hipEventRecord(f->e0, f->stream));
  HS_HIP(hs_undist_enqueue(u, f->stream, raw, nullptr, f->d_raw));
  return run_track(f, f->d_raw, max_l1_error, n_good);
}

// The same, with cvImgL copied device to device from a device image (include/hs_image.h) behind its last set.
int hs_flow_track_image(hs_flow* f, hs_image* im, float max_l1_error, int* n_good) {
  if (!f || !im) return hs::fail(HS_ERR_INVALID, "null argument");
  HsImageView v;
  HS_TRY(hs_image_view(im, f->device, f->W, f->H, 1, true, &v));
  HS_TRY(need_first(f));
  HS_HIP(hipSetDevice(f->device));
  HS_HIP(hipStreamWaitEvent(f->stream, v.ready, 0));
  HS_HIP(hipEventRecord(f->e0, f->stream));
  HS_HIP(hipMemcpyAsync(f->d_raw, v.img8, (size_t)f->W * f->H, hipMemcpyDeviceToDevice, f->stream));
  HS_HIP(hs_image_consumed(im, f->stream));
  return run_track(f, f->d_raw, max_l1_error, n_good);
}

// Initialize()'s first-frame branch with cvImgL copied device to device from a device image and the keys from the host.
int hs_flow_set_first_image(hs_flow* f, hs_image* im, int n, const float* xy) {
  if (!f || !im || (n > 0 && !xy)) return hs::fail(HS_ERR_INVALID, "null argument");
  if (n < 0 || n > f->cap)
    return hs::fail(HS_ERR_INVALID, std::to_string(n) + " points, capacity is " + std::to_string(f->cap));
  HsImageView v;
  HS_TRY(hs_image_view(im, f->device, f->W, f->H, 1, true, &v));
  HS_HIP(hipSetDevice(f->device));
  HS_HIP(hipStreamWaitEvent(f->stream, v.ready, 0));
  HS_HIP(hipMemcpyAsync(f->d_raw, v.img8, (size_t)f->W * f->H, hipMemcpyDeviceToDevice, f->stream));
  HS_HIP(hs_image_consumed(im, f->stream));
  if (n) HS_HIP(hipMemcpyAsync(f->d_first, xy, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, f->stream));
  return finish_first(f, f->d_raw, n);
}

int hs_flow_get(hs_flow* f, int* n, float* first_xy, float* prev_xy, float* xy, uint8_t* status, float* err,
                uint8_t* good) {
  if (!f) return hs::fail(HS_ERR_INVALID, "null flow");
  HS_HIP(hipSetDevice(f->device));
  if (n) *n = f->n;
  const size_t m = f->n;
  if (!m) return HS_OK;
  hipStream_t s = f->stream;
  const size_t pb = m * sizeof(float2);
  if (first_xy) HS_HIP(hipMemcpyAsync(first_xy, f->d_first, pb, hipMemcpyDeviceToHost, s));
  if (prev_xy) HS_HIP(hipMemcpyAsync(prev_xy, f->d_pts[f->pcur ^ 1], pb, hipMemcpyDeviceToHost, s));
  if (xy) HS_HIP(hipMemcpyAsync(xy, f->d_pts[f->pcur], pb, hipMemcpyDeviceToHost, s));
  if (status) HS_HIP(hipMemcpyAsync(status, f->d_status, m, hipMemcpyDeviceToHost, s));
  if (err) HS_HIP(hipMemcpyAsync(err, f->d_err, m * sizeof(float), hipMemcpyDeviceToHost, s));
  if (good) HS_HIP(hipMemcpyAsync(good, f->d_good, m, hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  return HS_OK;
}

int hs_flow_mean_flow(hs_flow* f, float* mean) {
  if (!f || !mean) return hs::fail(HS_ERR_INVALID, "null argument");
  if (!f->tracked) return hs::fail(HS_ERR_STATE, "no track yet: there is no flow to average");
  std::vector<float> prev(2 * (size_t)f->n), cur(2 * (size_t)f->n);
  std::vector<uint8_t> good(f->n);
  HS_TRY(hs_flow_get(f, nullptr, nullptr, prev.data(), cur.data(), nullptr, nullptr, good.data()));
  // accumulate(Median.begin(), Median.end(), 0): the initial value is an int, so every partial sum is truncated
  int acc = 0, count = 0;
  for (int i = 0; i < f->n; i++) {
    if (!good[i]) continue;
    const float dx = prev[2 * i] - cur[2 * i], dy = prev[2 * i + 1] - cur[2 * i + 1];
    const float norm = (float)std::sqrt((double)dx * dx + (double)dy * dy);
    acc = (int)((float)acc + norm);
    count++;
  }
  *mean = (float)acc / (float)count;
  return HS_OK;
}

int hs_flow_mean_flow_device(hs_flow* f, float* mean) {
  if (!f || !mean) return hs::fail(HS_ERR_INVALID, "null argument");
  if (!f->tracked) return hs::fail(HS_ERR_STATE, "no track yet: there is no flow to average");
  HS_HIP(hipSetDevice(f->device));
  HsFlowMeanArgs a;
  a.n = f->n;
  a.prev_xy = f->d_pts[f->pcur ^ 1];
  a.xy = f->d_pts[f->pcur];
  a.good = f->d_good;
  a.mean = f->d_mean;
  hipLaunchKernelGGL(hs_k_flow_mean, dim3(1), dim3(256), 0, f->stream, a);
  HS_HIP(hipGetLastError());
  HS_HIP(hipMemcpyAsync(f->h_mean, f->d_mean, sizeof(float), hipMemcpyDeviceToHost, f->stream));
  HS_HIP(hipStreamSynchronize(f->stream));
  *mean = *f->h_mean;
  return HS_OK;
}

int hs_flow_calc(hs_flow* f, const uint8_t* prev8, const uint8_t* next8, int n, const float* prev_xy,
                 const float* init_xy, float* xy_out, uint8_t* status_out, float* err_out) {
  if (!f || !prev8 || !next8 || (n > 0 && !prev_xy)) return hs::fail(HS_ERR_INVALID, "null argument");
  if (n < 0 || n > f->cap)
    return hs::fail(HS_ERR_INVALID, std::to_string(n) + " points, capacity is " + std::to_string(f->cap));
  HS_HIP(hipSetDevice(f->device));
  hipStream_t s = f->stream;
  const size_t area = (size_t)f->W * f->H, pb = (size_t)n * sizeof(float2);
  if (n) {
    HS_HIP(hipMemcpyAsync(f->d_cprev, prev_xy, pb, hipMemcpyHostToDevice, s));
    if (init_xy) HS_HIP(hipMemcpyAsync(f->d_cinit, init_xy, pb, hipMemcpyHostToDevice, s));
  }
  HS_HIP(hipEventRecord(f->e0, s));
  HS_HIP(hipMemcpyAsync(f->d_raw, prev8, area, hipMemcpyHostToDevice, s));
  HS_TRY(build_slot(f, 2, f->d_raw));
  HS_HIP(hipMemcpyAsync(f->d_raw, next8, area, hipMemcpyHostToDevice, s));  // behind slot 2's reads on the stream
  HS_TRY(build_slot(f, 3, f->d_raw));
  LkIo io;
  io.prev_xy = f->d_cprev;
  io.init_xy = init_xy ? f->d_cinit : nullptr;
  io.xy = f->d_cxy;
  io.status = f->d_cstatus;
  io.good = f->d_cgood;
  io.err = f->d_cerr;
  HS_TRY(enqueue_lk(f, 2, 3, n, io, INFINITY));
  if (n) {
    if (xy_out) HS_HIP(hipMemcpyAsync(xy_out, f->d_cxy, pb, hipMemcpyDeviceToHost, s));
    if (status_out) HS_HIP(hipMemcpyAsync(status_out, f->d_cstatus, n, hipMemcpyDeviceToHost, s));
    if (err_out) HS_HIP(hipMemcpyAsync(err_out, f->d_cerr, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
  }
  HS_TRY(finish(f));
  f->last[0] = 2;
  f->last[1] = 3;
  return HS_OK;
}

int hs_flow_get_pyramid(hs_flow* f, int which, int level, uint8_t* img_out, int16_t* deriv_out, int* w, int* h) {
  if (!f) return hs::fail(HS_ERR_INVALID, "null flow");
  if (which < 0 || which > 1) return hs::fail(HS_ERR_INVALID, "which must be 0 (previous) or 1 (next)");
  if (level < 0 || level >= f->lv.n)
    return hs::fail(HS_ERR_INVALID, "level " + std::to_string(level) + " does not exist: the image has " +
                                        std::to_string(f->lv.n));
  if (f->last[which] < 0) return hs::fail(HS_ERR_STATE, "no calc or track yet");
  HS_HIP(hipSetDevice(f->device));
  const int lw = f->lv.w[level], lh = f->lv.h[level], stride = lw + 2 * kFlowPad;
  if (w) *w = lw;
  if (h) *h = lh;
  const hs_flow_slot& sl = f->slot[f->last[which]];
  const size_t origin = (size_t)f->lv.off[level] + (size_t)kFlowPad * stride + kFlowPad;
  if (img_out)
    HS_HIP(hipMemcpy2DAsync(img_out, lw, sl.img + origin, stride, lw, lh, hipMemcpyDeviceToHost, f->stream));
  if (deriv_out)
    HS_HIP(hipMemcpy2DAsync(deriv_out, (size_t)lw * sizeof(short2), sl.deriv + origin, (size_t)stride * sizeof(short2),
                            (size_t)lw * sizeof(short2), lh, hipMemcpyDeviceToHost, f->stream));
  HS_HIP(hipStreamSynchronize(f->stream));
  return HS_OK;
}

int hs_flow_last_stats(hs_flow* f, double* ms, long long* iterations, int* levels) {
  if (!f) return hs::fail(HS_ERR_INVALID, "null flow");
  if (ms) *ms = f->last_ms;
  if (iterations) *iterations = f->last_iters;
  if (levels) *levels = f->lv.n;
  return HS_OK;
}

}  // extern "C"
