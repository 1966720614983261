// hs_trace.cpp — C-ABI implementation of the immature-point tracing boundary (include/hs_trace.h):
// tracer context, device SoA of ImmaturePoint state, ctor / traceOn / tally launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hs_ba.h"
#include "../../include/hs_trace.h"
#include "hs_ba_ctx.h"
#include "hs_env.h"
#include "hs_host.h"
#include "hs_trace_kernels.h"
#include "../../include/hs_undist.h"
#include "hs_undist_kernels.h"
#include "../../include/hs_extract.h"
#include "hs_extract_kernels.h"
#include "../../include/hs_image.h"
#include "hs_image_kernels.h"

#define HS_MAXF_ACT 8                        // activation window (nF <= 8 keyframes)
#define HS_ACT_LDS_MAP_MAX (156 * 1024)     // level-1 distance map in LDS up to this size

struct hs_tracer : hs::Device {
  hs_params P;
  hs::Pool pool;
  int W = 0, H = 0, cap = 0, n = 0;
  float4* d_host_img[HS_TRC_MAXHOST] = {nullptr};
  const float4** d_host_tab = nullptr;
  float4* d_new = nullptr;
  float* d_raw = nullptr;  // staging of a raw level-0 frame (hs_tracer_set_frame_raw)
  bool have_frame = false;
  hs_trace_host* d_hosts = nullptr;
  int* d_host = nullptr;
  float *d_u = nullptr, *d_v = nullptr, *d_color = nullptr, *d_weights = nullptr, *d_gradH = nullptr;
  float *d_energyTH = nullptr, *d_quality = nullptr, *d_idmin = nullptr, *d_idmax = nullptr;
  float *d_uv = nullptr, *d_interval = nullptr;
  uint8_t* d_status = nullptr;
  int* d_steps = nullptr;
  int* d_counts = nullptr;
  int* h_counts = nullptr;
  float last_ms = 0;
  long long last_steps = 0;
  bool stats_pending = false;
  bool tracing = false;  // HS_KTRACE=1 at creation: hs_k_act_select's profile on stderr
  int max_host = -1;  // largest host slot of the stored points
  float* d_type = nullptr;  // ImmaturePoint::my_type
  // point activation scratch (allocated by the first hs_tracer_activate)
  bool act_ready = false;
  int w1 = 0, h1 = 0, act_cap = 0;
  uint8_t* d_dist = nullptr;
  int *d_list_a = nullptr, *d_list_b = nullptr, *d_act_cnt = nullptr;
  hs_act_frame* d_act_frames = nullptr;
  hs_act_pair* d_act_pairs = nullptr;
  int* d_frame_of_slot = nullptr;
  int *d_order = nullptr, *d_cell = nullptr, *d_toopt = nullptr, *d_act_seeds = nullptr;
  uint8_t *d_cand = nullptr, *d_action = nullptr, *d_res_in = nullptr;
  float *d_frac = nullptr, *d_thr = nullptr, *d_act_idepth = nullptr;
  int* d_ap_frame = nullptr;
  float *d_ap_u = nullptr, *d_ap_v = nullptr, *d_ap_id = nullptr;
  // host mirror of d_host (a point's image slot): the BA hand-off names each activated point's window frame, and the
  // device compaction its survivors, without reading the slots back
  std::vector<int> h_host;
  // activation into a BA window and the device compaction (allocated by their first call)
  bool ba_ready = false;
  hipEvent_t ev_handoff = nullptr;      // tracer -> BA stream order (the staged points)
  uint8_t* h_act_rb = nullptr;          // pinned read-back: toOptimize [cap] ints | action [cap] | IN masks [cap]
  int* d_stage_pos = nullptr;           // hs_k_act_stage's ranks
  HsCmpPointSet alt{};                  // the compaction's second buffer set (swapped with the live one)
  int *d_cmp_pos = nullptr, *d_cmp_blk = nullptr;
  uint8_t *d_cmp_keep = nullptr, *d_cmp_drop = nullptr;
  bool action_valid = false;            // h_act_rb / d_action hold the last hs_tracer_activate_ba's actions of these points
  // what the last hs_tracer_activate_ba formed and read (hs_tracer_get_act_inputs)
  hs_ctx* in_ba = nullptr;
  unsigned in_seq = 0;
  int in_nF = 0, in_n_active = 0;
  float in_K4[4] = {0, 0, 0, 0};
  // what the last hs_tracer_trace_ba formed (hs_tracer_get_trace_inputs): the slots it wrote in d_hosts
  int trc_n_hosts = 0;
  bool trc_named[HS_TRC_MAXHOST] = {false};
};

static HsCmpPointSet live_set(hs_tracer* t) {
  return {t->d_host, t->d_u, t->d_v, t->d_color, t->d_weights, t->d_gradH, t->d_energyTH, t->d_quality, t->d_idmin,
          t->d_idmax, t->d_uv, t->d_interval, t->d_status, t->d_steps, t->d_type};
}

static int upload_img(hs_tracer* t, float4* dst, const float* src) {
  const size_t n = (size_t)t->W * t->H;
  std::vector<float4> tex(n);
  hs::texels_from_triplets(tex.data(), src, n);
  HS_HIP(hipMemcpyAsync(dst, tex.data(), n * sizeof(float4), hipMemcpyHostToDevice, t->stream));
  HS_HIP(hipStreamSynchronize(t->stream));
  return HS_OK;
}

static int sync_stats(hs_tracer* t) {
  if (!t->stats_pending) return HS_OK;
  HS_HIP(hipStreamSynchronize(t->stream));
  HS_HIP(hipEventElapsedTime(&t->last_ms, t->e0, t->e1));
  long long st = 0;
  memcpy(&st, t->h_counts + 6, sizeof(st));
  t->last_steps = st;
  t->stats_pending = false;
  return HS_OK;
}

static int launch_ctor(hs_tracer* t, int first, int n) {
  HsImmCtorArgs a;
  a.n = n;
  a.first = first;
  a.W = t->W;
  a.H = t->H;
  a.host_img = t->d_host_tab;
  a.host = t->d_host;
  a.u = t->d_u;
  a.v = t->d_v;
  a.outlierTHSumComponent = t->P.outlierTHSumComponent;
  a.outlierTH = t->P.outlierTH;
  a.overallEnergyTHWeight = t->P.overallEnergyTHWeight;
  a.color = t->d_color;
  a.weights = t->d_weights;
  a.gradH = t->d_gradH;
  a.energyTH = t->d_energyTH;
  a.quality = t->d_quality;
  a.idepth_min = t->d_idmin;
  a.idepth_max = t->d_idmax;
  a.status = t->d_status;
  a.uv = t->d_uv;
  a.interval = t->d_interval;
  hipLaunchKernelGGL(hs_k_imm_ctor, dim3((n + 255) / 256), dim3(256), 0, t->stream, a);
  HS_HIP(hipGetLastError());
  return HS_OK;
}

extern "C" {

int hs_tracer_create(hs_tracer** out, const hs_params* params, int device_id, int width, int height, int capacity) {
  if (!out) return hs::fail(HS_ERR_INVALID, "null out");
  *out = nullptr;
  if (width < 16 || height < 16 || capacity < 1) return hs::fail(HS_ERR_INVALID, "bad size / capacity");
  HS_TRY(hs::check_device(device_id));
  hs_tracer* t = new hs_tracer();
  if (params) t->P = *params;
  else hs_params_default(&t->P);
  t->W = width;
  t->H = height;
  t->cap = capacity;
  t->tracing = hs::env::ktrace();
  const size_t c = capacity;
  const int rc = [&]() -> int {
    hs::Pool& m = t->pool;
    HS_TRY(t->open(device_id));
    HS_TRY(m.alloc(&t->d_new, (size_t)width * height));
    HS_TRY(m.alloc_zero(&t->d_host_tab, HS_TRC_MAXHOST, t->stream));  // the kernels' stream
    HS_TRY(m.alloc(&t->d_hosts, HS_TRC_MAXHOST));
    HS_TRY(m.alloc(&t->d_host, c));
    HS_TRY(m.alloc(&t->d_u, c));
    HS_TRY(m.alloc(&t->d_v, c));
    HS_TRY(m.alloc(&t->d_color, 8 * c));
    HS_TRY(m.alloc(&t->d_weights, 8 * c));
    HS_TRY(m.alloc(&t->d_gradH, 4 * c));
    HS_TRY(m.alloc(&t->d_energyTH, c));
    HS_TRY(m.alloc(&t->d_quality, c));
    HS_TRY(m.alloc(&t->d_idmin, c));
    HS_TRY(m.alloc(&t->d_idmax, c));
    HS_TRY(m.alloc(&t->d_uv, 2 * c));
    HS_TRY(m.alloc(&t->d_interval, c));
    HS_TRY(m.alloc(&t->d_status, c));
    HS_TRY(m.alloc(&t->d_steps, c));
    HS_TRY(m.alloc(&t->d_type, c));
    HS_TRY(m.alloc(&t->d_counts, 8));
    HS_TRY(m.pinned(&t->h_counts, 8));
    return HS_OK;
  }();
  if (rc) hs_tracer_destroy(t);
  else *out = t;
  return rc;
}

void hs_tracer_destroy(hs_tracer* t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  if (t->stream) (void)hipStreamSynchronize(t->stream);
  t->pool.release_all();
  if (t->ev_handoff) (void)hipEventDestroy(t->ev_handoff);
  t->close();
  delete t;
}

// host slot `slot`'s image buffer, allocated and entered in the device table on first use
static int host_slot(hs_tracer* t, int slot) {
  if (t->d_host_img[slot]) return HS_OK;
  HS_TRY(t->pool.alloc(&t->d_host_img[slot], (size_t)t->W * t->H));
  // (the source is a member: it keeps its value and outlives the copy, whenever the stream gets to it)
  HS_HIP(hipMemcpyAsync(t->d_host_tab + slot, &t->d_host_img[slot], sizeof(float4*), hipMemcpyHostToDevice, t->stream));
  return HS_OK;
}

int hs_tracer_set_host_image(hs_tracer* t, int slot, const float* img) {
  if (!t || !img) return hs::fail(HS_ERR_INVALID, "null argument");
  if (slot < 0 || slot >= HS_TRC_MAXHOST) return hs::fail(HS_ERR_INVALID, "host slot out of range");
  HS_HIP(hipSetDevice(t->device));
  HS_TRY(host_slot(t, slot));
  return upload_img(t, t->d_host_img[slot], img);
}

int hs_tracer_clear(hs_tracer* t) {
  if (!t) return hs::fail(HS_ERR_INVALID, "null tracer");
  t->n = 0;
  t->max_host = -1;
  t->h_host.clear();
  t->action_valid = false;
  return HS_OK;
}

int hs_tracer_add_points(hs_tracer* t, int n, const int* host, const float* u, const float* v) {
  if (!t || (n > 0 && (!host || !u || !v))) return hs::fail(HS_ERR_INVALID, "null argument");
  if (n < 0 || t->n + n > t->cap) return hs::fail(HS_ERR_INVALID, "point capacity exceeded");
  if (n == 0) return HS_OK;
  for (int i = 0; i < n; i++) {
    // the ctor's BiLin taps reach 2 px around (u, v) plus one texel: reject points whose pattern leaves the image
    if (host[i] < 0 || host[i] >= HS_TRC_MAXHOST || !t->d_host_img[host[i]])
      return hs::fail(HS_ERR_INVALID, "point on a host slot without an image");
    if (!(u[i] >= 2 && v[i] >= 2 && u[i] < t->W - 3 && v[i] < t->H - 3))
      return hs::fail(HS_ERR_INVALID, "immature point too close to the image border");
  }
  HS_HIP(hipSetDevice(t->device));
  const int f = t->n;
  HS_HIP(hipMemcpyAsync(t->d_host + f, host, sizeof(int) * n, hipMemcpyHostToDevice, t->stream));
  HS_HIP(hipMemcpyAsync(t->d_u + f, u, sizeof(float) * n, hipMemcpyHostToDevice, t->stream));
  HS_HIP(hipMemcpyAsync(t->d_v + f, v, sizeof(float) * n, hipMemcpyHostToDevice, t->stream));
  const std::vector<float> ones(n, 1.f);
  HS_HIP(hipMemcpyAsync(t->d_type + f, ones.data(), sizeof(float) * n, hipMemcpyHostToDevice, t->stream));
  for (int i = 0; i < n; i++) t->max_host = std::max(t->max_host, host[i]);
  HS_TRY(launch_ctor(t, f, n));
  HS_HIP(hipStreamSynchronize(t->stream));  // host arrays may go away after return
  t->h_host.insert(t->h_host.end(), host, host + n);
  t->action_valid = false;
  t->n += n;
  return HS_OK;
}

int hs_tracer_add_keys(hs_tracer* t, hs_extractor* e, int slot, int* n_added) {
  if (!t || !e) return hs::fail(HS_ERR_INVALID, "null argument");
  if (slot < 0 || slot >= HS_TRC_MAXHOST || !t->d_host_img[slot])
    return hs::fail(HS_ERR_INVALID, "keys on a host slot without an image");
  int dev = 0, w = 0, h = 0, n = 0;
  const float *d_x = nullptr, *d_y = nullptr;
  hipEvent_t ready = nullptr;
  hs_extract_keys(e, &dev, &w, &h, &n, &d_x, &d_y, &ready);
  if (dev != t->device) return hs::fail(HS_ERR_INVALID, "extractor and tracer are on different devices");
  if (w != t->W || h != t->H) return hs::fail(HS_ERR_INVALID, "extractor size differs from the tracer's");
  if (t->n + n > t->cap) return hs::fail(HS_ERR_INVALID, "point capacity exceeded");
  if (n_added) *n_added = n;
  if (n == 0) return HS_OK;
  HS_HIP(hipSetDevice(t->device));
  const int f = t->n;
  // keys lie >= 19 px from the left and top edges and >= 18 px from the right and bottom ones (a fast extract keeps
  // x = W-19 / y = H-19, include/hs_extract.h): add_points' border rule, which needs 3 px, holds by construction
  HS_HIP(hipStreamWaitEvent(t->stream, ready, 0));
  HS_HIP(hipMemcpyAsync(t->d_u + f, d_x, sizeof(float) * n, hipMemcpyDeviceToDevice, t->stream));
  HS_HIP(hipMemcpyAsync(t->d_v + f, d_y, sizeof(float) * n, hipMemcpyDeviceToDevice, t->stream));
  HS_HIP(hs_extract_keys_consumed(e, t->stream));
  HS_HIP(hipMemsetD32Async((hipDeviceptr_t)(t->d_host + f), slot, n, t->stream));
  HS_HIP(hipMemsetD32Async((hipDeviceptr_t)(t->d_type + f), 0x3f800000, n, t->stream));  // my_type 1.f
  t->max_host = std::max(t->max_host, slot);
  HS_TRY(launch_ctor(t, f, n));
  t->h_host.insert(t->h_host.end(), (size_t)n, slot);
  t->action_valid = false;
  t->n += n;
  return HS_OK;
}

int hs_tracer_set_state(hs_tracer* t, const float* idepth_min, const float* idepth_max, const float* quality,
                        const uint8_t* status, const float* interval) {
  if (!t) return hs::fail(HS_ERR_INVALID, "null tracer");
  if (status)
    for (int i = 0; i < t->n; i++)
      if (status[i] > HS_IPS_UNINITIALIZED) return hs::fail(HS_ERR_INVALID, "bad ImmaturePointStatus");
  HS_HIP(hipSetDevice(t->device));
  const size_t n = t->n;
  if (idepth_min) HS_HIP(hipMemcpyAsync(t->d_idmin, idepth_min, 4 * n, hipMemcpyHostToDevice, t->stream));
  if (idepth_max) HS_HIP(hipMemcpyAsync(t->d_idmax, idepth_max, 4 * n, hipMemcpyHostToDevice, t->stream));
  if (quality) HS_HIP(hipMemcpyAsync(t->d_quality, quality, 4 * n, hipMemcpyHostToDevice, t->stream));
  if (status) HS_HIP(hipMemcpyAsync(t->d_status, status, n, hipMemcpyHostToDevice, t->stream));
  if (interval) HS_HIP(hipMemcpyAsync(t->d_interval, interval, 4 * n, hipMemcpyHostToDevice, t->stream));
  HS_HIP(hipStreamSynchronize(t->stream));
  return HS_OK;
}

int hs_tracer_set_frame(hs_tracer* t, const float* img) {
  if (!t || !img) return hs::fail(HS_ERR_INVALID, "null argument");
  HS_HIP(hipSetDevice(t->device));
  int rc = upload_img(t, t->d_new, img);
  if (rc) return rc;
  t->have_frame = true;
  return HS_OK;
}

int hs_tracer_set_frame_raw(hs_tracer* t, const float* img) {
  if (!t || !img) return hs::fail(HS_ERR_INVALID, "null argument");
  HS_HIP(hipSetDevice(t->device));
  if (!t->d_raw) HS_TRY(t->pool.alloc(&t->d_raw, (size_t)t->W * t->H));
  HS_HIP(hipMemcpyAsync(t->d_raw, img, sizeof(float) * t->W * t->H, hipMemcpyHostToDevice, t->stream));
  float4* lv[1] = {t->d_new};
  HS_HIP(hs_img_build(t->stream, t->W, t->H, 1, lv, nullptr, nullptr, t->d_raw, nullptr));
  HS_HIP(hipStreamSynchronize(t->stream));
  t->have_frame = true;
  return HS_OK;
}

int hs_tracer_set_frame_u8(hs_tracer* t, hs_undistorter* u, const uint8_t* raw) {
  if (!t || !u || !raw) return hs::fail(HS_ERR_INVALID, "null argument");
  HS_TRY(hs_undist_match(u, t->device, t->W, t->H));
  HS_HIP(hipSetDevice(t->device));
  HsUndistArgs tab;
  hs_undist_tables(u, &tab);
  HS_HIP(hs_undist_upload(u, t->stream, raw));
  float4* lv[1] = {t->d_new};
  HS_HIP(hs_img_build(t->stream, t->W, t->H, 1, lv, nullptr, nullptr, nullptr, &tab));
  HS_HIP(hipStreamSynchronize(t->stream));
  t->have_frame = true;
  return HS_OK;
}

// level 0 of a device image (include/hs_image.h) into one of the tracer's own level-0 buffers, device to device
// behind the image's last set; no host wait (every reader of dst runs on the tracer's stream)
static int copy_image_level0(hs_tracer* t, float4* dst, hs_image* im, const HsImageView& v) {
  HS_HIP(hipStreamWaitEvent(t->stream, v.ready, 0));
  HS_HIP(hipMemcpyAsync(dst, v.lvl[0], sizeof(float4) * (size_t)t->W * t->H, hipMemcpyDeviceToDevice, t->stream));
  HS_HIP(hs_image_consumed(im, t->stream));
  return HS_OK;
}

int hs_tracer_set_frame_image(hs_tracer* t, hs_image* im) {
  if (!t || !im) return hs::fail(HS_ERR_INVALID, "null argument");
  HsImageView v;
  HS_TRY(hs_image_view(im, t->device, t->W, t->H, 1, false, &v));
  HS_HIP(hipSetDevice(t->device));
  HS_TRY(copy_image_level0(t, t->d_new, im, v));
  t->have_frame = true;
  return HS_OK;
}

int hs_tracer_set_host_image_from(hs_tracer* t, int slot, hs_image* im) {
  if (!t || !im) return hs::fail(HS_ERR_INVALID, "null argument");
  if (slot < 0 || slot >= HS_TRC_MAXHOST) return hs::fail(HS_ERR_INVALID, "host slot out of range");
  HsImageView v;
  HS_TRY(hs_image_view(im, t->device, t->W, t->H, 1, false, &v));
  HS_HIP(hipSetDevice(t->device));
  HS_TRY(host_slot(t, slot));
  return copy_image_level0(t, t->d_host_img[slot], im, v);
}

// traceOn of every point against t->d_new with the (KRKi, Kt, aff) records in t->d_hosts, then the tallies: the one
// launch hs_tracer_trace and hs_tracer_trace_ba share
static int trace_launch(hs_tracer* t, int counts6[6]) {
  HsTraceArgs a;
  a.n = t->n;
  a.W = t->W;
  a.H = t->H;
  a.img = t->d_new;
  a.hosts = t->d_hosts;
  a.host = t->d_host;
  a.u = t->d_u;
  a.v = t->d_v;
  a.color = t->d_color;
  a.weights = t->d_weights;
  a.gradH = t->d_gradH;
  a.energyTH = t->d_energyTH;
  a.quality = t->d_quality;
  a.idepth_min = t->d_idmin;
  a.idepth_max = t->d_idmax;
  a.status = t->d_status;
  a.uv = t->d_uv;
  a.interval = t->d_interval;
  a.steps = t->d_steps;
  a.huberTH = t->P.huberTH;
  a.maxPixSearch = t->P.maxPixSearch;
  a.slackInterval = t->P.trace_slackInterval;
  a.stepsize = t->P.trace_stepsize;
  a.minImprovementFactor = t->P.trace_minImprovementFactor;
  a.GNThreshold = t->P.trace_GNThreshold;
  a.extraSlackOnTH = t->P.trace_extraSlackOnTH;
  a.minTraceTestRadius = t->P.minTraceTestRadius;
  a.GNIterations = t->P.trace_GNIterations;
  HS_HIP(hipEventRecord(t->e0, t->stream));
  if (t->n > 0) {
    hipLaunchKernelGGL(hs_k_trace_on, dim3((t->n + 3) / 4), dim3(256), 0, t->stream, a);
    HS_HIP(hipGetLastError());
  }
  HS_HIP(hipEventRecord(t->e1, t->stream));
  hipLaunchKernelGGL(hs_k_trace_count, dim3(1), dim3(1024), 0, t->stream, t->n, t->d_status, t->d_steps,
                     t->d_counts);
  HS_HIP(hipGetLastError());
  HS_HIP(hipMemcpyAsync(t->h_counts, t->d_counts, sizeof(int) * 8, hipMemcpyDeviceToHost, t->stream));
  t->stats_pending = true;
  if (!counts6) return HS_OK;  // asynchronous: hs_tracer_last_stats / get_points synchronise
  HS_TRY(sync_stats(t));
  for (int k = 0; k < 6; k++) counts6[k] = t->h_counts[k];
  return HS_OK;
}

int hs_tracer_trace(hs_tracer* t, int n_hosts, const hs_trace_host* hosts, int counts6[6]) {
  if (!t || (n_hosts > 0 && !hosts)) return hs::fail(HS_ERR_INVALID, "null argument");
  if (n_hosts < 0 || n_hosts > HS_TRC_MAXHOST) return hs::fail(HS_ERR_INVALID, "n_hosts out of range");
  if (!t->have_frame) return hs::fail(HS_ERR_STATE, "no frame to trace on (hs_tracer_set_frame)");
  HS_HIP(hipSetDevice(t->device));
  if (t->n > 0) {
    // every point's host slot must have its (KRKi, Kt, aff)
    if (t->max_host >= n_hosts) return hs::fail(HS_ERR_INVALID, "a point's host slot has no hs_trace_host entry");
    HS_HIP(hipMemcpyAsync(t->d_hosts, hosts, sizeof(hs_trace_host) * n_hosts, hipMemcpyHostToDevice, t->stream));
  }
  return trace_launch(t, counts6);
}

int hs_tracer_get_points(hs_tracer* t, int* n, uint8_t* status, float* idepth_min, float* idepth_max, float* quality,
                         float* uv, float* interval, float* energyTH, float* color, float* weights, float* gradH) {
  if (!t) return hs::fail(HS_ERR_INVALID, "null tracer");
  HS_HIP(hipSetDevice(t->device));
  HS_HIP(hipStreamSynchronize(t->stream));
  const size_t m = t->n;
  if (n) *n = t->n;
  if (status) HS_HIP(hipMemcpy(status, t->d_status, m, hipMemcpyDeviceToHost));
  if (idepth_min) HS_HIP(hipMemcpy(idepth_min, t->d_idmin, 4 * m, hipMemcpyDeviceToHost));
  if (idepth_max) HS_HIP(hipMemcpy(idepth_max, t->d_idmax, 4 * m, hipMemcpyDeviceToHost));
  if (quality) HS_HIP(hipMemcpy(quality, t->d_quality, 4 * m, hipMemcpyDeviceToHost));
  if (uv) HS_HIP(hipMemcpy(uv, t->d_uv, 8 * m, hipMemcpyDeviceToHost));
  if (interval) HS_HIP(hipMemcpy(interval, t->d_interval, 4 * m, hipMemcpyDeviceToHost));
  if (energyTH) HS_HIP(hipMemcpy(energyTH, t->d_energyTH, 4 * m, hipMemcpyDeviceToHost));
  if (color) HS_HIP(hipMemcpy(color, t->d_color, 32 * m, hipMemcpyDeviceToHost));
  if (weights) HS_HIP(hipMemcpy(weights, t->d_weights, 32 * m, hipMemcpyDeviceToHost));
  if (gradH) HS_HIP(hipMemcpy(gradH, t->d_gradH, 16 * m, hipMemcpyDeviceToHost));
  return HS_OK;
}

int hs_tracer_last_stats(hs_tracer* t, double* ms, long long* search_steps) {
  if (!t) return hs::fail(HS_ERR_INVALID, "null tracer");
  HS_HIP(hipSetDevice(t->device));
  HS_TRY(sync_stats(t));
  if (ms) *ms = t->last_ms;
  if (search_steps) *search_steps = t->last_steps;
  return HS_OK;
}

int hs_tracer_reinit(hs_tracer* t) {
  if (!t) return hs::fail(HS_ERR_INVALID, "null tracer");
  if (t->n == 0) return HS_OK;
  HS_HIP(hipSetDevice(t->device));
  return launch_ctor(t, 0, t->n);
}

int hs_tracer_set_types(hs_tracer* t, const float* my_type) {
  if (!t || (t->n > 0 && !my_type)) return hs::fail(HS_ERR_INVALID, "null argument");
  HS_HIP(hipSetDevice(t->device));
  HS_HIP(hipMemcpyAsync(t->d_type, my_type, sizeof(float) * t->n, hipMemcpyHostToDevice, t->stream));
  HS_HIP(hipStreamSynchronize(t->stream));
  return HS_OK;
}

static int act_alloc(hs_tracer* t) {
  if (t->act_ready) return HS_OK;
  t->w1 = t->W >> 1;
  t->h1 = t->H >> 1;
  const size_t wh1 = (size_t)t->w1 * t->h1, c = t->cap;
  hs::Pool& m = t->pool;
  HS_TRY(m.alloc(&t->d_dist, (wh1 + 3) & ~(size_t)3));
  HS_TRY(m.alloc(&t->d_list_a, wh1));
  HS_TRY(m.alloc(&t->d_list_b, wh1));
  HS_TRY(m.alloc(&t->d_act_cnt, 2));
  HS_TRY(m.alloc(&t->d_act_frames, HS_MAXF_ACT));
  HS_TRY(m.alloc(&t->d_act_pairs, HS_MAXF_ACT * HS_MAXF_ACT));
  HS_TRY(m.alloc(&t->d_frame_of_slot, HS_TRC_MAXHOST));
  HS_TRY(m.alloc(&t->d_order, c));
  HS_TRY(m.alloc(&t->d_cell, c));
  HS_TRY(m.alloc(&t->d_toopt, c + 64));  // + the greedy loop's 64 scratch slots
  HS_TRY(m.alloc(&t->d_act_seeds, 2 * c));  // seeds | the select's pending list
  HS_TRY(m.alloc(&t->d_cand, c));
  HS_TRY(m.alloc(&t->d_action, c));
  HS_TRY(m.alloc(&t->d_res_in, c));
  HS_TRY(m.alloc(&t->d_frac, c));
  HS_TRY(m.alloc(&t->d_thr, c));
  HS_TRY(m.alloc(&t->d_act_idepth, c));
  t->act_ready = true;
  return HS_OK;
}

static int act_points_alloc(hs_tracer* t, int n) {
  if (n <= t->act_cap) return HS_OK;
  hs::Pool& m = t->pool;
  m.release(&t->d_ap_frame);
  m.release(&t->d_ap_u);
  m.release(&t->d_ap_v);
  m.release(&t->d_ap_id);
  t->act_cap = 0;
  HS_TRY(m.alloc(&t->d_ap_frame, n));
  HS_TRY(m.alloc(&t->d_ap_u, n));
  HS_TRY(m.alloc(&t->d_ap_v, n));
  HS_TRY(m.alloc(&t->d_ap_id, n));
  t->act_cap = n;
  return HS_OK;
}

// System::activatePointsMT :332-352 (float currentMinActDist, double constants as in the reference)
static void update_min_act_dist(const hs_params& P, int nPoints, float& d) {
  if (nPoints < P.desiredPointDensity * 0.66) d -= 0.8;
  if (nPoints < P.desiredPointDensity * 0.8) d -= 0.5;
  else if (nPoints < P.desiredPointDensity * 0.9) d -= 0.2;
  else if (nPoints < P.desiredPointDensity) d -= 0.1;
  if (nPoints > P.desiredPointDensity * 1.5) d += 0.8;
  if (nPoints > P.desiredPointDensity * 1.3) d += 0.5;
  if (nPoints > P.desiredPointDensity * 1.15) d += 0.2;
  if (nPoints > P.desiredPointDensity) d += 0.1;
  if (d < 0) d = 0;
  if (d > 4) d = 4;
}

// the kernels of one activatePointsMT call: seed, cand, dist, select, dist, optimize.  The frames / pairs / slot
// table / order are on the device already; the active points are read where r says (the tracer's own upload, or a BA
// context's point set).  Synchronises once, for the candidate count.
struct ActRun {
  const float* K4;
  int nF, n_active;
  const int* d_frame;
  const float *d_u, *d_v, *d_idepth;
  int m;            // loop-order entries
  bool has_order;   // t->d_order holds them (else storage order)
  float cmad;       // currentMinActDist after its update
};

static int act_launch(hs_tracer* t, const ActRun& r, int* n_toopt_out) {
  hipStream_t s = t->stream;
  const int wh1 = t->w1 * t->h1, nF = r.nF, m = r.m;
  HS_HIP(hipMemsetAsync(t->d_dist, 0xff, (wh1 + 3) & ~3, s));
  HS_HIP(hipMemsetAsync(t->d_act_cnt, 0, sizeof(int) * 2, s));
  HS_HIP(hipMemsetAsync(t->d_action, HS_ACT_KEEP, std::max(1, t->n), s));
  HS_HIP(hipMemsetAsync(t->d_res_in, 0, std::max(1, t->n), s));

  HsActSeedArgs sa;
  sa.n = r.n_active;
  sa.newest = nF - 1;
  sa.w1 = t->w1;
  sa.h1 = t->h1;
  sa.frames = t->d_act_frames;
  sa.frame = r.d_frame;
  sa.u = r.d_u;
  sa.v = r.d_v;
  sa.idepth = r.d_idepth;
  sa.dist = t->d_dist;
  sa.list = t->d_list_a;
  sa.count = t->d_act_cnt;
  if (r.n_active > 0) {
    hipLaunchKernelGGL(hs_k_act_seed, dim3((r.n_active + 255) / 256), dim3(256), 0, s, sa);
    HS_HIP(hipGetLastError());
  }
  HsActCandArgs ca;
  ca.m = m;
  ca.newest = nF - 1;
  ca.w1 = t->w1;
  ca.h1 = t->h1;
  ca.minTraceQuality = t->P.minTraceQuality;
  ca.currentMinActDist = r.cmad;
  ca.order = r.has_order ? t->d_order : nullptr;
  ca.frame_of_slot = t->d_frame_of_slot;
  ca.frames = t->d_act_frames;
  ca.host = t->d_host;
  ca.u = t->d_u;
  ca.v = t->d_v;
  ca.idepth_min = t->d_idmin;
  ca.idepth_max = t->d_idmax;
  ca.quality = t->d_quality;
  ca.interval = t->d_interval;
  ca.my_type = t->d_type;
  ca.status = t->d_status;
  ca.cand = t->d_cand;
  ca.cell = t->d_cell;
  ca.frac = t->d_frac;
  ca.thr = t->d_thr;
  ca.action = t->d_action;
  if (m > 0) {
    hipLaunchKernelGGL(hs_k_act_cand, dim3((m + 255) / 256), dim3(256), 0, s, ca);
    HS_HIP(hipGetLastError());
  }
  // makeDistanceMap's growDistBFS over the seeds
  HsActDistArgs ma;
  ma.w1 = t->w1;
  ma.h1 = t->h1;
  ma.mode = 0;
  ma.n_tiles_x = (t->w1 - 2 + 15) / 16;
  ma.n_tiles = ma.n_tiles_x * ((t->h1 - 2 + 15) / 16);
  const int border_waves = 2 * ((t->w1 + 63) / 64) + 2 * ((t->h1 - 2 + 63) / 64);
  const int dist_blocks = ma.n_tiles + (border_waves + 3) / 4;
  ma.seeds = t->d_list_a;
  ma.n_seeds = t->d_act_cnt;
  ma.init = t->d_dist;
  ma.out = reinterpret_cast<uint8_t*>(t->d_list_b);
  hipLaunchKernelGGL(hs_k_act_dist, dim3(dist_blocks), dim3(256), 0, s, ma);
  HS_HIP(hipGetLastError());
  HsActSelectArgs se;
  se.m = m;
  se.w1 = t->w1;
  se.h1 = t->h1;
  const size_t map_bytes = (size_t)((wh1 + 3) & ~3);
  se.lds_map = map_bytes <= HS_ACT_LDS_MAP_MAX ? 1 : 0;
  se.order = r.has_order ? t->d_order : nullptr;
  se.cand = t->d_cand;
  se.cell = t->d_cell;
  se.frac = t->d_frac;
  se.thr = t->d_thr;
  se.dist = t->d_dist;
  se.map0 = reinterpret_cast<uint8_t*>(t->d_list_b);
  se.seeds = t->d_act_seeds;
  se.plist = t->d_act_seeds + t->cap;
  se.toopt = t->d_toopt;
  se.n_toopt = t->d_act_cnt + 1;
  hs::Pool scratch;  // freed on every return path
  long long* d_prof = nullptr;
  if (t->tracing) HS_TRY(scratch.alloc(&d_prof, 11));
  se.prof = d_prof;
  const size_t lds = se.lds_map ? map_bytes : 0;
  if (lds > 65536)
    HS_HIP(hipFuncSetAttribute((const void*)hs_k_act_select, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(hs_k_act_select, dim3(1), dim3(1024), lds, s, se);
  HS_HIP(hipGetLastError());
  HsActDistArgs fa = ma;  // the map the greedy loop leaves
  fa.mode = 1;
  fa.seeds = se.seeds;
  fa.n_seeds = se.n_toopt;
  fa.init = ma.out;
  fa.out = t->d_dist;
  hipLaunchKernelGGL(hs_k_act_dist, dim3(dist_blocks), dim3(256), 0, s, fa);
  HS_HIP(hipGetLastError());
  int cnt[2] = {0, 0};
  HS_HIP(hipMemcpyAsync(cnt, t->d_act_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  const int n_toopt = cnt[1];
  if (d_prof) {
    long long pr[11];
    HS_HIP(hipMemcpy(pr, d_prof, sizeof(pr), hipMemcpyDeviceToHost));
    fprintf(stderr, "hs act prof: prologue %.1f us, greedy %.1f us (decisions %.1f, folds %.1f of which border %.1f; "
            "wall_clock64 @100 MHz), %d selected; %lld batches, %lld seed patches of radius %lld; core clock %.0f MHz\n",
            (pr[1] - pr[0]) * 1e-2, (pr[2] - pr[1]) * 1e-2, pr[8] * 1e-2, pr[9] * 1e-2, pr[10] * 1e-2, n_toopt, pr[3],
            pr[4], pr[5],
            (double)(pr[7] - pr[6]) / ((pr[2] - pr[1]) * 1e-2));
  }
  if (n_toopt > 0) {
    HsActOptArgs oa;
    oa.n = n_toopt;
    oa.nF = nF;
    oa.W = t->W;
    oa.H = t->H;
    oa.fxl = r.K4[0];
    oa.fyl = r.K4[1];
    oa.cxl = r.K4[2];
    oa.cyl = r.K4[3];
    oa.fxli = 1.0f / r.K4[0];
    oa.fyli = 1.0f / r.K4[1];
    oa.huberTH = t->P.huberTH;
    oa.minIdepthH_act = t->P.minIdepthH_act;
    oa.GNIts = t->P.GNItsOnPointActivation;
    oa.toopt = t->d_toopt;
    oa.frame_of_slot = t->d_frame_of_slot;
    oa.frames = t->d_act_frames;
    oa.pairs = t->d_act_pairs;
    oa.img = t->d_host_tab;
    oa.host = t->d_host;
    oa.u = t->d_u;
    oa.v = t->d_v;
    oa.idepth_min = t->d_idmin;
    oa.idepth_max = t->d_idmax;
    oa.color = t->d_color;
    oa.weights = t->d_weights;
    oa.energyTH = t->d_energyTH;
    oa.action = t->d_action;
    oa.idepth_out = t->d_act_idepth;
    oa.res_in = t->d_res_in;
    hipLaunchKernelGGL(hs_k_act_optimize, dim3((n_toopt + 3) / 4), dim3(256), 0, s, oa);
    HS_HIP(hipGetLastError());
  }
  *n_toopt_out = n_toopt;
  return HS_OK;
}

int hs_tracer_activate(hs_tracer* t, const float K4[4], int nF, const hs_act_frame* frames, const hs_act_pair* pairs,
                       int n_active, const int* act_frame, const float* act_u, const float* act_v,
                       const float* act_idepth, int ef_nPoints, float* currentMinActDist, int n_order,
                       const int* order, uint8_t* action, float* idepth, uint8_t* res_in, int* activated,
                       int* n_activated) {
  if (!t || !K4 || !frames || !pairs || !currentMinActDist) return hs::fail(HS_ERR_INVALID, "null argument");
  if (nF < 2 || nF > HS_MAXF_ACT) return hs::fail(HS_ERR_INVALID, "window size out of range (2..8 keyframes)");
  if (n_active < 0 || (n_active > 0 && (!act_frame || !act_u || !act_v || !act_idepth)))
    return hs::fail(HS_ERR_INVALID, "bad active point arrays");
  if (!(K4[0] > 0) || !(K4[1] > 0)) return hs::fail(HS_ERR_INVALID, "bad intrinsics");
  std::vector<int> fos(HS_TRC_MAXHOST, -1);
  for (int f = 0; f < nF; f++) {
    const int sl = frames[f].slot;
    if (sl < 0 || sl >= HS_TRC_MAXHOST || !t->d_host_img[sl]) return hs::fail(HS_ERR_INVALID, "window frame without an image slot");
    if (fos[sl] >= 0) return hs::fail(HS_ERR_INVALID, "two window frames on one slot");
    fos[sl] = f;
  }
  for (int i = 0; i < n_active; i++)
    if (act_frame[i] < 0 || act_frame[i] >= nF) return hs::fail(HS_ERR_INVALID, "active point on no window frame");
  const int m = order ? n_order : t->n;
  if (order) {
    if (n_order < 0 || n_order > t->n) return hs::fail(HS_ERR_INVALID, "bad n_order");
    std::vector<char> seen(t->n, 0);
    for (int j = 0; j < n_order; j++) {
      if (order[j] < 0 || order[j] >= t->n || seen[order[j]]) return hs::fail(HS_ERR_INVALID, "order is not a subset permutation");
      seen[order[j]] = 1;
    }
  }
  HS_HIP(hipSetDevice(t->device));
  HS_TRY(sync_stats(t));
  HS_TRY(act_alloc(t));
  HS_TRY(act_points_alloc(t, std::max(1, n_active)));
  update_min_act_dist(t->P, ef_nPoints, *currentMinActDist);
  t->action_valid = false;
  hipStream_t s = t->stream;
  HS_HIP(hipMemcpyAsync(t->d_act_frames, frames, sizeof(hs_act_frame) * nF, hipMemcpyHostToDevice, s));
  HS_HIP(hipMemcpyAsync(t->d_act_pairs, pairs, sizeof(hs_act_pair) * nF * nF, hipMemcpyHostToDevice, s));
  HS_HIP(hipMemcpyAsync(t->d_frame_of_slot, fos.data(), sizeof(int) * HS_TRC_MAXHOST, hipMemcpyHostToDevice, s));
  if (order && m > 0) HS_HIP(hipMemcpyAsync(t->d_order, order, sizeof(int) * m, hipMemcpyHostToDevice, s));
  if (n_active > 0) {
    HS_HIP(hipMemcpyAsync(t->d_ap_frame, act_frame, sizeof(int) * n_active, hipMemcpyHostToDevice, s));
    HS_HIP(hipMemcpyAsync(t->d_ap_u, act_u, sizeof(float) * n_active, hipMemcpyHostToDevice, s));
    HS_HIP(hipMemcpyAsync(t->d_ap_v, act_v, sizeof(float) * n_active, hipMemcpyHostToDevice, s));
    HS_HIP(hipMemcpyAsync(t->d_ap_id, act_idepth, sizeof(float) * n_active, hipMemcpyHostToDevice, s));
  }
  int n_toopt = 0;
  const ActRun run{K4, nF, n_active, t->d_ap_frame, t->d_ap_u, t->d_ap_v, t->d_ap_id, m, order != nullptr,
                   *currentMinActDist};
  HS_TRY(act_launch(t, run, &n_toopt));
  const size_t n = t->n;
  std::vector<uint8_t> act(std::max<size_t>(1, n));
  std::vector<int> toopt(std::max(1, n_toopt));
  HS_HIP(hipMemcpyAsync(act.data(), t->d_action, n, hipMemcpyDeviceToHost, s));
  if (n_toopt > 0) HS_HIP(hipMemcpyAsync(toopt.data(), t->d_toopt, sizeof(int) * n_toopt, hipMemcpyDeviceToHost, s));
  if (idepth && n) HS_HIP(hipMemcpyAsync(idepth, t->d_act_idepth, sizeof(float) * n, hipMemcpyDeviceToHost, s));
  if (res_in && n) HS_HIP(hipMemcpyAsync(res_in, t->d_res_in, n, hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  if (action && n) memcpy(action, act.data(), n);
  int na = 0;
  for (int k = 0; k < n_toopt; k++)
    if (act[toopt[k]] == HS_ACT_ACTIVATED) {
      if (activated) activated[na] = toopt[k];
      na++;
    }
  if (idepth)  // the idepth output is defined for activated points only
    for (size_t i = 0; i < n; i++)
      if (act[i] != HS_ACT_ACTIVATED) idepth[i] = 0.f;
  if (n_activated) *n_activated = na;
  return HS_OK;
}

int hs_tracer_get_distance_map(hs_tracer* t, float* dist) {
  if (!t || !dist) return hs::fail(HS_ERR_INVALID, "null argument");
  if (!t->act_ready) return hs::fail(HS_ERR_STATE, "no activation has run");
  HS_HIP(hipSetDevice(t->device));
  const size_t wh1 = (size_t)t->w1 * t->h1;
  std::vector<uint8_t> b(wh1);
  HS_HIP(hipStreamSynchronize(t->stream));
  HS_HIP(hipMemcpy(b.data(), t->d_dist, wh1, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < wh1; i++) dist[i] = b[i] == 255 ? 1000.f : (float)b[i];
  return HS_OK;
}

// stable compaction of every per-point array (a host round trip: once per keyframe)
extern "C++" template <typename T>
static int compact_array(hs_tracer* t, T* d, int per, const std::vector<int>& keep_idx) {
  const size_t n = t->n;
  std::vector<T> h(n * per), o(keep_idx.size() * per);
  if (n) HS_HIP(hipMemcpy(h.data(), d, sizeof(T) * n * per, hipMemcpyDeviceToHost));
  for (size_t k = 0; k < keep_idx.size(); k++)
    for (int c = 0; c < per; c++) o[k * per + c] = h[(size_t)keep_idx[k] * per + c];
  if (!o.empty()) {  // on the kernels' stream; o lives until the copy has landed
    HS_HIP(hipMemcpyAsync(d, o.data(), sizeof(T) * o.size(), hipMemcpyHostToDevice, t->stream));
    HS_HIP(hipStreamSynchronize(t->stream));
  }
  return HS_OK;
}

int hs_tracer_compact(hs_tracer* t, const uint8_t* keep) {
  if (!t || (t->n > 0 && !keep)) return hs::fail(HS_ERR_INVALID, "null argument");
  HS_HIP(hipSetDevice(t->device));
  HS_TRY(sync_stats(t));
  HS_HIP(hipStreamSynchronize(t->stream));
  std::vector<int> idx;
  for (int i = 0; i < t->n; i++)
    if (keep[i]) idx.push_back(i);
  HS_TRY(compact_array(t, t->d_host, 1, idx));
  HS_TRY(compact_array(t, t->d_u, 1, idx));
  HS_TRY(compact_array(t, t->d_v, 1, idx));
  HS_TRY(compact_array(t, t->d_color, 8, idx));
  HS_TRY(compact_array(t, t->d_weights, 8, idx));
  HS_TRY(compact_array(t, t->d_gradH, 4, idx));
  HS_TRY(compact_array(t, t->d_energyTH, 1, idx));
  HS_TRY(compact_array(t, t->d_quality, 1, idx));
  HS_TRY(compact_array(t, t->d_idmin, 1, idx));
  HS_TRY(compact_array(t, t->d_idmax, 1, idx));
  HS_TRY(compact_array(t, t->d_uv, 2, idx));
  HS_TRY(compact_array(t, t->d_interval, 1, idx));
  HS_TRY(compact_array(t, t->d_status, 1, idx));
  HS_TRY(compact_array(t, t->d_steps, 1, idx));
  HS_TRY(compact_array(t, t->d_type, 1, idx));
  std::vector<int> hosts(idx.size());
  if (!idx.empty()) HS_HIP(hipMemcpy(hosts.data(), t->d_host, sizeof(int) * idx.size(), hipMemcpyDeviceToHost));
  t->max_host = -1;
  for (int h : hosts) t->max_host = std::max(t->max_host, h);
  t->h_host.swap(hosts);
  t->action_valid = false;
  t->n = (int)idx.size();
  return HS_OK;
}

// ---- activation into a BA window, compaction on the device ------------------------------------------------------

static int act_ba_alloc(hs_tracer* t) {
  if (t->ba_ready) return HS_OK;
  const size_t c = t->cap;
  hs::Pool& m = t->pool;
  if (!t->ev_handoff) HS_HIP(hipEventCreateWithFlags(&t->ev_handoff, hipEventDisableTiming));
  HS_TRY(m.pinned(&t->h_act_rb, 6 * c));
  HS_TRY(m.alloc(&t->d_stage_pos, c));
  HsCmpPointSet& a = t->alt;
  HS_TRY(m.alloc(&a.host, c));
  HS_TRY(m.alloc(&a.u, c));
  HS_TRY(m.alloc(&a.v, c));
  HS_TRY(m.alloc(&a.color, 8 * c));
  HS_TRY(m.alloc(&a.weights, 8 * c));
  HS_TRY(m.alloc(&a.gradH, 4 * c));
  HS_TRY(m.alloc(&a.energyTH, c));
  HS_TRY(m.alloc(&a.quality, c));
  HS_TRY(m.alloc(&a.idmin, c));
  HS_TRY(m.alloc(&a.idmax, c));
  HS_TRY(m.alloc(&a.uv, 2 * c));
  HS_TRY(m.alloc(&a.interval, c));
  HS_TRY(m.alloc(&a.status, c));
  HS_TRY(m.alloc(&a.steps, c));
  HS_TRY(m.alloc(&a.type, c));
  HS_TRY(m.alloc(&t->d_cmp_pos, c));
  HS_TRY(m.alloc(&t->d_cmp_blk, (c + HS_CMP_NT - 1) / HS_CMP_NT));
  HS_TRY(m.alloc(&t->d_cmp_keep, c));
  HS_TRY(m.alloc(&t->d_cmp_drop, HS_TRC_MAXHOST));
  t->ba_ready = true;
  return HS_OK;
}

// keep (host flags, one per point; null: the last hs_tracer_activate_ba's action == HS_ACT_KEEP) and not
// drop_slot[slot]: the survivors into the second buffer set in their order, then the sets swap.  No read-back: the
// host decides the same flags from its mirror of the points' slots.
static int compact_on_device(hs_tracer* t, const uint8_t* keep, const uint8_t* drop_slot) {
  const int n = t->n;
  const uint8_t* act = t->h_act_rb + 4 * (size_t)t->cap;
  std::vector<int> hosts;
  hosts.reserve(n);
  for (int i = 0; i < n; i++) {
    const int h = t->h_host[i];
    const bool k = (keep ? keep[i] != 0 : act[i] == HS_ACT_KEEP) && !(drop_slot && drop_slot[h]);
    if (k) hosts.push_back(h);
  }
  if (n > 0) {
    hipStream_t s = t->stream;
    HsCmpArgs a;
    a.n = n;
    a.keep_in = nullptr;
    if (keep) {
      HS_HIP(hipMemcpyAsync(t->d_cmp_keep, keep, n, hipMemcpyHostToDevice, s));
      a.keep_in = t->d_cmp_keep;
    }
    a.action = t->d_action;
    a.drop_slot = nullptr;
    if (drop_slot) {
      HS_HIP(hipMemcpyAsync(t->d_cmp_drop, drop_slot, HS_TRC_MAXHOST, hipMemcpyHostToDevice, s));
      a.drop_slot = t->d_cmp_drop;
    }
    a.pos = t->d_cmp_pos;
    a.blk = t->d_cmp_blk;
    a.from = live_set(t);
    a.to = t->alt;
    const int nblk = (n + HS_CMP_NT - 1) / HS_CMP_NT;
    hipLaunchKernelGGL(hs_k_cmp_flags, dim3(nblk), dim3(HS_CMP_NT), 0, s, a);
    HS_HIP(hipGetLastError());
    hipLaunchKernelGGL(hs_k_cmp_scan, dim3(1), dim3(1024), 0, s, a, nblk);
    HS_HIP(hipGetLastError());
    hipLaunchKernelGGL(hs_k_cmp_scatter, dim3((int)(((size_t)n * 8 + 255) / 256)), dim3(256), 0, s, a);
    HS_HIP(hipGetLastError());
    if (keep || drop_slot) HS_HIP(hipStreamSynchronize(s));  // the caller's flag arrays may go away after return
    HsCmpPointSet& b = t->alt;
    std::swap(t->d_host, b.host);
    std::swap(t->d_u, b.u);
    std::swap(t->d_v, b.v);
    std::swap(t->d_color, b.color);
    std::swap(t->d_weights, b.weights);
    std::swap(t->d_gradH, b.gradH);
    std::swap(t->d_energyTH, b.energyTH);
    std::swap(t->d_quality, b.quality);
    std::swap(t->d_idmin, b.idmin);
    std::swap(t->d_idmax, b.idmax);
    std::swap(t->d_uv, b.uv);
    std::swap(t->d_interval, b.interval);
    std::swap(t->d_status, b.status);
    std::swap(t->d_steps, b.steps);
    std::swap(t->d_type, b.type);
  }
  t->max_host = -1;
  for (int h : hosts) t->max_host = std::max(t->max_host, h);
  t->h_host.swap(hosts);
  t->n = (int)t->h_host.size();
  t->action_valid = false;
  return HS_OK;
}

int hs_tracer_compact_device(hs_tracer* t, const uint8_t* keep, const uint8_t* drop_slot, int* n_left) {
  if (!t) return hs::fail(HS_ERR_INVALID, "null tracer");
  if (!keep && t->n > 0 && !t->action_valid)
    return hs::fail(HS_ERR_STATE, "no keep flags and no hs_tracer_activate_ba actions of these points");
  HS_HIP(hipSetDevice(t->device));
  HS_TRY(sync_stats(t));
  HS_TRY(act_alloc(t));
  HS_TRY(act_ba_alloc(t));
  HS_TRY(compact_on_device(t, keep, drop_slot));
  if (n_left) *n_left = t->n;
  return HS_OK;
}

int hs_tracer_activate_ba(hs_tracer* t, hs_ctx* ba, int nF, const int* slots, const int* flagged_for_marg,
                          float* currentMinActDist, int n_order, const int* order, int compact,
                          const uint8_t* drop_slot, uint8_t* action_out, int* handles_out, int* n_activated,
                          int* n_deleted) {
  if (!t || !ba || !slots || !flagged_for_marg || !currentMinActDist) return hs::fail(HS_ERR_INVALID, "null argument");
  if (ba->comm_lost) return hs::fail(HS_ERR_RCCL, "communicator aborted by an earlier call (a peer rank failed)");
  if (ba->multi_rank()) return hs::fail(HS_ERR_STATE, "hs_tracer_activate_ba needs a single-rank BA context");
  if (ba->device != t->device) return hs::fail(HS_ERR_INVALID, "tracer and BA context on different devices");
  if (!ba->d_state || !ba->haveCam) return hs::fail(HS_ERR_STATE, "the BA context has no window");
  if (ba->cam.width != t->W || ba->cam.height != t->H) return hs::fail(HS_ERR_INVALID, "image size mismatch");
  const int wnF = ba->incremental ? (int)ba->wframes.size() : ba->nF;
  if (nF < 2 || nF > HS_MAXF_ACT) return hs::fail(HS_ERR_INVALID, "window size out of range (2..8 keyframes)");
  if (nF != wnF) return hs::fail(HS_ERR_INVALID, "nF differs from the BA window's number of frames");
  std::vector<int> fos(HS_TRC_MAXHOST, -1);
  for (int f = 0; f < nF; f++) {
    const int sl = slots[f];
    if (sl < 0 || sl >= HS_TRC_MAXHOST || !t->d_host_img[sl])
      return hs::fail(HS_ERR_INVALID, "window frame without an image slot");
    if (fos[sl] >= 0) return hs::fail(HS_ERR_INVALID, "two window frames on one slot");
    fos[sl] = f;
  }
  const int m = order ? n_order : t->n;
  if (order) {
    if (n_order < 0 || n_order > t->n) return hs::fail(HS_ERR_INVALID, "bad n_order");
    std::vector<char> seen(t->n, 0);
    for (int j = 0; j < n_order; j++) {
      if (order[j] < 0 || order[j] >= t->n || seen[order[j]])
        return hs::fail(HS_ERR_INVALID, "order is not a subset permutation");
      seen[order[j]] = 1;
    }
  }
  HS_HIP(hipSetDevice(t->device));
  HS_TRY(sync_stats(t));
  HS_TRY(act_alloc(t));
  HS_TRY(act_ba_alloc(t));
  // The newest frame (and whatever else is pending: the last keyframe's removals) becomes visible on the device: the
  // pending edits are committed first; the points activated here are committed by the caller's makeIDX.
  HS_TRY(hs_ba_make_idx(ba, nullptr, nullptr, nullptr));
  if (!ba->h_state_valid) HS_TRY(hs::fetch_state(ba));  // the calibration (a commit with a new frame left it valid)
  float K4[4];
  for (int k = 0; k < 4; k++) K4[k] = ba->h_state->calib.value_scaledf[k];
  if (!(K4[0] > 0) || !(K4[1] > 0)) return hs::fail(HS_ERR_STATE, "bad intrinsics in the BA context");
  const int n_active = ba->nP;
  float cmad = *currentMinActDist;
  update_min_act_dist(t->P, n_active, cmad);
  hipStream_t s = t->stream;
  // the tracer's stream after the BA's: the committed point set and the frames' state
  HS_HIP(hipEventRecord(ba->ev_ready, ba->stream));
  HS_HIP(hipStreamWaitEvent(s, ba->ev_ready, 0));
  HsActFormArgs fa;
  fa.nF = nF;
  for (int f = 0; f < 8; f++) {
    fa.slot[f] = f < nF ? slots[f] : -1;
    fa.flagged[f] = f < nF ? flagged_for_marg[f] : 0;
  }
  fa.st = ba->d_state;
  fa.frames = t->d_act_frames;
  fa.pairs = t->d_act_pairs;
  hipLaunchKernelGGL(hs_k_act_form, dim3(1), dim3(64), 0, s, fa);
  HS_HIP(hipGetLastError());
  HS_HIP(hipMemcpyAsync(t->d_frame_of_slot, fos.data(), sizeof(int) * HS_TRC_MAXHOST, hipMemcpyHostToDevice, s));
  if (order && m > 0) HS_HIP(hipMemcpyAsync(t->d_order, order, sizeof(int) * m, hipMemcpyHostToDevice, s));
  t->in_ba = ba;
  t->in_seq = ba->commit_seq;
  t->in_nF = nF;
  t->in_n_active = n_active;
  memcpy(t->in_K4, K4, sizeof(K4));
  t->action_valid = false;
  int n_toopt = 0;
  const ActRun run{K4, nF, n_active, ba->d_pt_host, ba->d_u, ba->d_v, ba->d_idepth, m, order != nullptr, cmad};
  HS_TRY(act_launch(t, run, &n_toopt));
  // the structural read-back: actions, IN masks, the toOptimize list (pinned, one sync)
  const size_t n = t->n, cap = t->cap;
  int* h_toopt = reinterpret_cast<int*>(t->h_act_rb);
  uint8_t* h_action = t->h_act_rb + 4 * cap;
  uint8_t* h_res_in = t->h_act_rb + 5 * cap;
  if (n) {
    HS_HIP(hipMemcpyAsync(h_action, t->d_action, n, hipMemcpyDeviceToHost, s));
    HS_HIP(hipMemcpyAsync(h_res_in, t->d_res_in, n, hipMemcpyDeviceToHost, s));
  }
  if (n_toopt > 0) HS_HIP(hipMemcpyAsync(h_toopt, t->d_toopt, sizeof(int) * n_toopt, hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  std::vector<int> host_frame;
  std::vector<uint8_t> masks;
  for (int k = 0; k < n_toopt; k++) {
    const int i = h_toopt[k];
    if (h_action[i] != HS_ACT_ACTIVATED) continue;
    host_frame.push_back(fos[t->h_host[i]]);
    masks.push_back(h_res_in[i]);
  }
  const int na = (int)host_frame.size();
  if (hs::mirror_points(ba) + na > ba->cap_P || ba->n_dev_staged + na > ba->cap_P)
    return hs::fail(HS_ERR_NOMEM, "activated points exceed the BA context's point capacity (hs_ba_reserve)");
  const int base = ba->n_dev_staged;
  HS_TRY(hs::stage_activated(ba, na, host_frame.data(), masks.data(), handles_out));
  if (na > 0) {
    HsActStageArgs sa;
    sa.n = n_toopt;
    sa.base = base;
    sa.toopt = t->d_toopt;
    sa.action = t->d_action;
    sa.idepth = t->d_act_idepth;
    sa.u = t->d_u;
    sa.v = t->d_v;
    sa.color = t->d_color;
    sa.weights = t->d_weights;
    sa.pos = t->d_stage_pos;
    sa.out = ba->d_act_stage;
    hipLaunchKernelGGL(hs_k_act_stage, dim3(1), dim3(1024), 0, s, sa);
    HS_HIP(hipGetLastError());
    // the BA's commit gathers the staged points: its stream after the tracer's
    HS_HIP(hipEventRecord(t->ev_handoff, s));
    HS_HIP(hipStreamWaitEvent(ba->stream, t->ev_handoff, 0));
  }
  *currentMinActDist = cmad;
  if (action_out && n) memcpy(action_out, h_action, n);
  int nd = 0;
  for (size_t i = 0; i < n; i++) nd += h_action[i] == HS_ACT_DELETED;
  if (n_activated) *n_activated = na;
  if (n_deleted) *n_deleted = nd;
  t->action_valid = true;
  if (compact) HS_TRY(compact_on_device(t, nullptr, drop_slot));
  return HS_OK;
}

int hs_tracer_get_act_inputs(hs_tracer* t, hs_ctx* ba, float K4[4], int* nF, hs_act_frame* frames, hs_act_pair* pairs,
                             int* n_active, int* act_frame, float* act_u, float* act_v, float* act_idepth) {
  if (!t || !ba) return hs::fail(HS_ERR_INVALID, "null argument");
  if (t->in_ba != ba || !t->in_nF) return hs::fail(HS_ERR_STATE, "no hs_tracer_activate_ba with this BA context");
  HS_HIP(hipSetDevice(t->device));
  HS_HIP(hipStreamSynchronize(t->stream));
  if (K4) memcpy(K4, t->in_K4, sizeof(t->in_K4));
  if (nF) *nF = t->in_nF;
  if (n_active) *n_active = t->in_n_active;
  const int f = t->in_nF;
  if (frames) HS_HIP(hipMemcpy(frames, t->d_act_frames, sizeof(hs_act_frame) * f, hipMemcpyDeviceToHost));
  if (pairs) HS_HIP(hipMemcpy(pairs, t->d_act_pairs, sizeof(hs_act_pair) * f * f, hipMemcpyDeviceToHost));
  if (act_frame || act_u || act_v || act_idepth) {
    // the active points were read where they lie in the BA's point set: gone with its next commit
    if (ba->commit_seq != t->in_seq)
      return hs::fail(HS_ERR_STATE, "the BA window was committed since the activation: its point arrays moved");
    const size_t n = t->in_n_active;
    HS_TRY(hs::wait_stream(ba));
    if (n && act_frame) HS_HIP(hipMemcpy(act_frame, ba->d_pt_host, 4 * n, hipMemcpyDeviceToHost));
    if (n && act_u) HS_HIP(hipMemcpy(act_u, ba->d_u, 4 * n, hipMemcpyDeviceToHost));
    if (n && act_v) HS_HIP(hipMemcpy(act_v, ba->d_v, 4 * n, hipMemcpyDeviceToHost));
    if (n && act_idepth) HS_HIP(hipMemcpy(act_idepth, ba->d_idepth, 4 * n, hipMemcpyDeviceToHost));
  }
  return HS_OK;
}

// ---- traceNewCoarse whose window is a BA context's ---------------------------------------------------------------

int hs_tracer_trace_ba(hs_tracer* t, hs_ctx* ba, int nF, const int* slots, const double new_worldToCam[7],
                       const double new_aff_g2l[2], float new_ab_exposure, int counts6[6]) {
  if (!t || !ba || !slots || !new_worldToCam || !new_aff_g2l) return hs::fail(HS_ERR_INVALID, "null argument");
  if (ba->comm_lost) return hs::fail(HS_ERR_RCCL, "communicator aborted by an earlier call (a peer rank failed)");
  if (ba->multi_rank()) return hs::fail(HS_ERR_STATE, "hs_tracer_trace_ba needs a single-rank BA context");
  if (ba->device != t->device) return hs::fail(HS_ERR_INVALID, "tracer and BA context on different devices");
  if (!ba->d_state || !ba->haveCam) return hs::fail(HS_ERR_STATE, "the BA context has no window");
  if (ba->cam.width != t->W || ba->cam.height != t->H) return hs::fail(HS_ERR_INVALID, "image size mismatch");
  const int wnF = ba->incremental ? (int)ba->wframes.size() : ba->nF;
  if (nF < 1 || nF > HS_MAXF || nF != wnF)
    return hs::fail(HS_ERR_INVALID, "nF differs from the BA window's number of frames");
  if (!t->have_frame) return hs::fail(HS_ERR_STATE, "no frame to trace on (hs_tracer_set_frame)");
  bool named[HS_TRC_MAXHOST] = {false};
  int n_hosts = 0;
  for (int f = 0; f < nF; f++) {
    const int sl = slots[f];
    if (sl < 0 || sl >= HS_TRC_MAXHOST) return hs::fail(HS_ERR_INVALID, "window frame's slot out of range");
    if (named[sl]) return hs::fail(HS_ERR_INVALID, "two window frames on one slot");
    named[sl] = true;
    n_hosts = std::max(n_hosts, sl + 1);
  }
  // every point's host slot must be a window frame's (the host mirror of the points' slots: no read-back)
  for (int i = 0; i < t->n; i++)
    if (!named[t->h_host[i]]) return hs::fail(HS_ERR_INVALID, "an immature point on a slot that is no window frame's");
  HS_HIP(hipSetDevice(t->device));
  // The frames are read at their committed index, which pending removals and point edits leave as it is (the steady
  // state: the last keyframe's hs_ba_remove_frame is still uncommitted), so those commit nothing here; a frame
  // inserted since the last commit is on the device only after it.
  bool inserted = false;
  if (ba->incremental)
    for (int f = 0; f < nF; f++) inserted = inserted || ba->wframes[f].committed < 0;
  if (inserted) HS_TRY(hs_ba_make_idx(ba, nullptr, nullptr, nullptr));
  HsTrcFormArgs fa;
  fa.nF = nF;
  for (int f = 0; f < 8; f++) {
    fa.idx[f] = f < nF ? (ba->incremental ? ba->wframes[f].committed : f) : 0;
    fa.slot[f] = f < nF ? slots[f] : 0;
    if (fa.idx[f] < 0 || fa.idx[f] >= HS_MAXF) return hs::fail(HS_ERR_STATE, "a window frame has no committed index");
  }
  memcpy(fa.new_worldToCam, new_worldToCam, sizeof(fa.new_worldToCam));
  fa.new_aff[0] = new_aff_g2l[0];
  fa.new_aff[1] = new_aff_g2l[1];
  fa.new_exposure = new_ab_exposure;
  fa.st = ba->d_state;
  fa.hosts = t->d_hosts;
  hipStream_t s = t->stream;
  // the tracer's stream after the BA's: the frames' state as the last GN step / commit left it
  HS_HIP(hipEventRecord(ba->ev_ready, ba->stream));
  HS_HIP(hipStreamWaitEvent(s, ba->ev_ready, 0));
  hipLaunchKernelGGL(hs_k_trc_form, dim3(1), dim3(64), 0, s, fa);
  HS_HIP(hipGetLastError());
  t->trc_n_hosts = n_hosts;
  memcpy(t->trc_named, named, sizeof(named));
  return trace_launch(t, counts6);
}

int hs_tracer_get_trace_inputs(hs_tracer* t, int* n_hosts, hs_trace_host* hosts) {
  if (!t) return hs::fail(HS_ERR_INVALID, "null tracer");
  if (!t->trc_n_hosts) return hs::fail(HS_ERR_STATE, "no hs_tracer_trace_ba has run");
  if (n_hosts) *n_hosts = t->trc_n_hosts;
  if (!hosts) return HS_OK;
  HS_HIP(hipSetDevice(t->device));
  HS_HIP(hipStreamSynchronize(t->stream));
  HS_HIP(hipMemcpy(hosts, t->d_hosts, sizeof(hs_trace_host) * t->trc_n_hosts, hipMemcpyDeviceToHost));
  for (int sl = 0; sl < t->trc_n_hosts; sl++)  // slots of no window frame: nothing was formed there
    if (!t->trc_named[sl]) memset(&hosts[sl], 0, sizeof(hs_trace_host));
  return HS_OK;
}

// test hook (not in the header, no device work): hs_host_math.h's make_trace_host on the host -- the inline
// hs_k_trc_form runs.  The host frames come from a device-state blob (hs_debug_get_state) at the indices idx [nF]
// (NULL: 0 .. nF-1), or, with state == NULL, from nF poses as hs_debug_act_inputs takes them; the new frame from its
// worldToCam [7], aff_g2l (a, b) and exposure.  Out: hosts [nF], in frame order.
int hs_debug_trace_hosts(const void* state, int nF, const int* idx, const double* worldToCam, const double* aff,
                         const float* exposure, const float* K4, const double* new_worldToCam, const double* new_aff,
                         float new_exposure, hs_trace_host* hosts) {
  if (nF < 1 || nF > HS_MAXF || !new_worldToCam || !new_aff || !hosts) return hs::fail(HS_ERR_INVALID, "bad argument");
  const hs::SE3 nw = hs::SE3::fromData(new_worldToCam);
  if (state) {
    const HsDevState* S = static_cast<const HsDevState*>(state);
    for (int f = 0; f < nF; f++) {
      const int k = idx ? idx[f] : f;
      if (k < 0 || k >= HS_MAXF) return hs::fail(HS_ERR_INVALID, "frame index out of range");
      hs::make_trace_host(S->frames[k], nw, new_exposure, new_aff[0], new_aff[1], S->calib, &hosts[f]);
    }
    return HS_OK;
  }
  if (!worldToCam || !aff || !exposure || !K4) return hs::fail(HS_ERR_INVALID, "bad argument");
  hs::CalibH cal;
  for (int k = 0; k < 4; k++) cal.value_scaledf[k] = K4[k];
  for (int f = 0; f < nF; f++) {
    hs::FrameH fr;
    fr.PRE_worldToCam = hs::SE3::fromData(worldToCam + 7 * f);
    fr.PRE_camToWorld = fr.PRE_worldToCam.inverse();
    fr.state_scaled[6] = aff[2 * f];
    fr.state_scaled[7] = aff[2 * f + 1];
    fr.ab_exposure = exposure[f];
    hs::make_trace_host(fr, nw, new_exposure, new_aff[0], new_aff[1], cal, &hosts[f]);
  }
  return HS_OK;
}

// test hook (not in the header, no device work): hs_host_math.h's make_act_* on the host -- the inlines
// hs_k_act_form runs.  The frames come from a device-state blob (hs_debug_get_state), or, with state == NULL, from
// nF poses: worldToCam [nF][7] (SE3 data, taken as PRE_worldToCam), aff [nF][2] (aff_g2l a, b), exposure [nF] and the
// level-0 K4.  Out: frames [nF] (slot / flag 0), pairs [nF*nF], kk [18] = K[1] | Ki[0].
int hs_debug_act_inputs(const void* state, int nF, const double* worldToCam, const double* aff, const float* exposure,
                        const float* K4, hs_act_frame* frames, hs_act_pair* pairs, float* kk) {
  if (nF < 1 || nF > HS_MAXF || !frames || !pairs) return hs::fail(HS_ERR_INVALID, "bad argument");
  std::vector<hs::FrameH> fr(nF);
  hs::CalibH cal;
  if (state) {
    const HsDevState* S = static_cast<const HsDevState*>(state);
    for (int f = 0; f < nF; f++) fr[f] = S->frames[f];
    cal = S->calib;
  } else {
    if (!worldToCam || !aff || !exposure || !K4) return hs::fail(HS_ERR_INVALID, "bad argument");
    for (int f = 0; f < nF; f++) {
      fr[f].PRE_worldToCam = hs::SE3::fromData(worldToCam + 7 * f);
      fr[f].PRE_camToWorld = fr[f].PRE_worldToCam.inverse();
      fr[f].state_scaled[6] = aff[2 * f];
      fr[f].state_scaled[7] = aff[2 * f + 1];
      fr[f].ab_exposure = exposure[f];
    }
    for (int k = 0; k < 4; k++) cal.value_scaledf[k] = K4[k];
  }
  float K1[9], Ki0[9];
  hs::make_act_K(cal, K1, Ki0);
  if (kk) {
    memcpy(kk, K1, sizeof(K1));
    memcpy(kk + 9, Ki0, sizeof(Ki0));
  }
  for (int h = 0; h < nF; h++) {
    frames[h].slot = 0;
    frames[h].flagged_for_marg = 0;
    hs::make_act_frame(fr[h], fr[nF - 1], K1, Ki0, frames[h].KRKi, frames[h].Kt);
    for (int t = 0; t < nF; t++) {
      hs_act_pair& p = pairs[h * nF + t];
      hs::make_act_pair(fr[h], fr[t], p.RTll, p.tTll, p.aff);
    }
  }
  return HS_OK;
}

}  // extern "C"
