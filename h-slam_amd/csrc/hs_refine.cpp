// hs_refine.cpp — C-ABI implementation of the DirectRefinement boundary (include/hs_refine.h): refiner
// context, device frames and point state (structure of arrays), and the LM step launches (one kernel per
// iteration, enqueued in batches; the device-side control block decides and stops).  Also the initializer hand-off of
// include/hs_init.h: the frames from a device image, the points from the flow context's first-frame keys, and
// System::InitFromInitializer's point loop into a BA window.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hs_init.h"
#include "../../include/hs_refine.h"
#include "hs_ba_ctx.h"
#include "hs_env.h"
#include "hs_flow_kernels.h"
#include "hs_host.h"
#include "hs_image_kernels.h"
#include "hs_init_kernels.h"
#include "hs_init_rule.h"
#include "hs_refine_kernels.h"
#include "hs_twoview_kernels.h"

namespace {
// Eigen compute_inverse_size3 in double (CalibData: pyrKi[0] = pyrK[0].inverse(), Include/CalibData.h:150)
void inv3d(const double m[9], double r[9]) {
  auto M = [&](int i, int j) { return m[i * 3 + j]; };
  auto cof = [&](int i, int j) {
    int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return M(i1, j1) * M(i2, j2) - M(i1, j2) * M(i2, j1);
  };
  const double c00 = cof(0, 0), c10 = cof(1, 0), c20 = cof(2, 0);
  const double invdet = 1.0 / (c00 * M(0, 0) + c10 * M(1, 0) + c20 * M(2, 0));
  r[0] = c00 * invdet; r[1] = c10 * invdet; r[2] = c20 * invdet;
  r[3] = cof(0, 1) * invdet; r[4] = cof(1, 1) * invdet; r[5] = cof(2, 1) * invdet;
  r[6] = cof(0, 2) * invdet; r[7] = cof(1, 2) * invdet; r[8] = cof(2, 2) * invdet;
}
}  // namespace

// per-point planes of the device state block (floats unless noted)
enum { PF_U, PF_V, PF_INVZ, PF_ID, PF_IDN, PF_IR, PF_E0, PF_E1, PF_EN0, PF_EN1, PF_LH, PF_LHN, PF_MS, PF_JB0 = PF_MS + 1,
       PF_COUNT = PF_JB0 + 20 };

struct hs_refiner : hs::Device {
  hs::Pool pool;
  int W = 0, H = 0;
  double K4[4] = {0, 0, 0, 0};
  double Ki[9];
  float4* d_img1 = nullptr;
  float4* d_img2 = nullptr;
  float expo1 = 0, expo2 = 0;
  bool have1 = false, have2 = false;  // FirstFrame / SecondFrame set (independently: hs_init.h)
  int n = 0, cap = 0;
  float* d_pf = nullptr;     // PF_COUNT planes of cap floats
  uint8_t* d_pb = nullptr;   // tri | good | good_new, cap bytes each
  int jb_sel = 0;
  HsRefCtl* d_ctl = nullptr;
  HsRefCtl* h_ctl = nullptr;
  int* h_flags = nullptr;
  double* d_part = nullptr;  // [nblocks][HS_REF_NRED]
  int* d_ticket = nullptr;
  float* d_log = nullptr;
  int last_iters = 0;
  bool tracing = false;          // HS_KTRACE=1 at creation
  long long* d_trace = nullptr;  // tracing: per-block stamps of each step launch, dumped to stderr
  double last_ms = 0;
  // hs_refiner_seed_ba (allocated by its first call, regrown with the point count)
  int seed_cap = 0;
  uint8_t* d_why = nullptr;
  uint8_t* h_why = nullptr;  // pinned
  int* d_nseed = nullptr;
  hipEvent_t ev_handoff = nullptr;  // refiner -> BA stream order (the staged points)
};

static HsRefPoints points_of(hs_refiner* r) {
  HsRefPoints p;
  const size_t c = (size_t)r->cap;
  float* f = r->d_pf;
  p.u = f + PF_U * c; p.v = f + PF_V * c; p.invz = f + PF_INVZ * c;
  p.idepth = f + PF_ID * c; p.idepth_new = f + PF_IDN * c; p.iR = f + PF_IR * c;
  p.energy = f + PF_E0 * c;        // [2][n]: planes E0 | E1 are contiguous only when n == cap, so n = cap below
  p.energy_new = f + PF_EN0 * c;
  p.lastH = f + PF_LH * c; p.lastH_new = f + PF_LHN * c; p.maxstep = f + PF_MS * c;
  p.jb[0] = f + PF_JB0 * c; p.jb[1] = f + (PF_JB0 + 10) * c;
  p.tri = r->d_pb; p.good = r->d_pb + c; p.good_new = r->d_pb + 2 * c;
  return p;
}

static HsRefArgs make_args(hs_refiner* r, int mode) {
  HsRefArgs a;
  std::memset(&a, 0, sizeof(a));
  a.p = points_of(r);
  a.n = r->n;
  a.W = r->W; a.H = r->H;
  a.mode = mode;
  a.nblocks = (r->n + HS_REF_PPB - 1) / HS_REF_PPB;
  a.fx = (float)r->K4[0]; a.fy = (float)r->K4[1]; a.cx = (float)r->K4[2]; a.cy = (float)r->K4[3];
  for (int q = 0; q < 9; q++) a.Ki[q] = r->Ki[q];
  a.img1 = r->d_img1;
  a.img2 = r->d_img2;
  a.huberTH = 9.f;                  // setting_huberTH (Src/Settings.cpp:68)
  a.outlierTH = 12 * 12;            // setting_outlierTH (Src/Settings.cpp:65)
  a.jb_sel0 = r->jb_sel;
  a.ctl = r->d_ctl;
  a.part = r->d_part;
  a.ticket = r->d_ticket;
  a.log = r->d_log;
  a.trace = r->d_trace;
  return a;
}

static int enqueue(hs_refiner* r, const HsRefArgs& a) {
  hipLaunchKernelGGL(hs_k_refine_step, dim3(a.nblocks), dim3(256), 0, r->stream, a);
  HS_HIP(hipGetLastError());
  return HS_OK;
}

static int dump_trace(hs_refiner* r, int nb, int launch_no) {
  std::vector<long long> t((size_t)nb * 16);
  HS_HIP(hipMemcpyAsync(t.data(), r->d_trace, t.size() * sizeof(long long), hipMemcpyDeviceToHost, r->stream));
  HS_HIP(hipStreamSynchronize(r->stream));
  int khz = 0;
  HS_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, r->device));
  const double us = khz > 0 ? 1e3 / khz : 0.01;
  long long t0 = t[0];
  for (int b = 0; b < nb; b++) t0 = std::min(t0, t[(size_t)b * 16]);
  for (int k = 0; k < 16; k++) {
    std::vector<double> v;
    for (int b = 0; b < nb; b++) {
      const long long x = t[(size_t)b * 16 + k];
      if (x >= t0) v.push_back((x - t0) * us);
    }
    if (v.empty()) continue;
    std::sort(v.begin(), v.end());
    std::fprintf(stderr, "[hs refine trace] launch %d cp%d n %3zu min %7.2f med %7.2f max %7.2f us\n", launch_no, k,
                 v.size(), v.front(), v[v.size() / 2], v.back());
  }
  HS_HIP(hipMemsetAsync(r->d_trace, 0, t.size() * sizeof(long long), r->stream));
  return HS_OK;
}

static int read_ctl(hs_refiner* r) {
  HS_HIP(hipMemcpyAsync(r->h_ctl, r->d_ctl, sizeof(HsRefCtl), hipMemcpyDeviceToHost, r->stream));
  HS_HIP(hipStreamSynchronize(r->stream));
  return HS_OK;
}

static int check_ready(hs_refiner* r) {
  if (!r->have1 || !r->have2) return hs::fail(HS_ERR_STATE, "both frames first (hs_refiner_set_frames, or hs_refiner_set_first_image and _set_second_image)");
  if (r->n <= 0) return hs::fail(HS_ERR_STATE, "hs_refiner_set_points / hs_refiner_set_points_flow first");
  HS_HIP(hipSetDevice(r->device));
  return HS_OK;
}

// resetPoints + one calcResAndGS at (T, aff)
static int run_calc(hs_refiner* r, const double T7[7], const double aff[2]) {
  HS_TRY(check_ready(r));
  HsRefArgs a = make_args(r, HS_REF_CALC);
  hs_ref_pass_consts(T7, aff, r->Ki, r->n, &a.pc0);
  HS_HIP(hipEventRecord(r->e0, r->stream));
  HS_TRY(enqueue(r, a));
  HS_HIP(hipEventRecord(r->e1, r->stream));
  HS_TRY(read_ctl(r));
  float ms = 0;
  HS_HIP(hipEventElapsedTime(&ms, r->e0, r->e1));
  r->last_ms = ms;
  return HS_OK;
}

// Refine: the first pass, then LM steps enqueued in batches until the device sets done, then the final applyStep
static int run_refine(hs_refiner* r, const double T7[7], const double aff[2]) {
  HS_TRY(check_ready(r));
  HsRefArgs a = make_args(r, HS_REF_INIT);
  hs_ref_pass_consts(T7, aff, r->Ki, r->n, &a.pc0);
  for (int q = 0; q < 7; q++) a.T0[q] = T7[q];
  a.aff0[0] = aff[0];
  a.aff0[1] = aff[1];
  HS_HIP(hipEventRecord(r->e0, r->stream));
  HS_TRY(enqueue(r, a));
  HsRefArgs it = make_args(r, HS_REF_ITER);
  int launched = 0, batch = 4;
  if (r->d_trace) batch = 1;
  for (;;) {
    for (int k = 0; k < batch; k++) HS_TRY(enqueue(r, it));
    if (r->d_trace && launched < 3) HS_TRY(dump_trace(r, it.nblocks, launched));
    launched += batch;
    HS_HIP(hipMemcpyAsync(&r->h_flags[0], &r->d_ctl->done, sizeof(int), hipMemcpyDeviceToHost, r->stream));
    HS_HIP(hipStreamSynchronize(r->stream));
    if (r->h_flags[0]) break;
    if (launched > HS_REF_MAXLOG + 8) return hs::fail(HS_ERR_STATE, "refine did not stop within the iteration cap");
    if (!r->d_trace) batch = std::min(2 * batch, 32);
  }
  HS_TRY(enqueue(r, make_args(r, HS_REF_FINAL)));  // the pending applyStep + optReg of the last accepted pass
  HS_HIP(hipEventRecord(r->e1, r->stream));
  HS_TRY(read_ctl(r));
  float ms = 0;
  HS_HIP(hipEventElapsedTime(&ms, r->e0, r->e1));
  r->last_ms = ms;
  r->jb_sel = r->h_ctl->jb_sel ^ r->h_ctl->apply_prev;
  r->last_iters = r->h_ctl->iteration + 1;
  return HS_OK;
}

// the state block of n points (the refiner then holds no points until the caller sets r->n)
static int alloc_points(hs_refiner* r, int n) {
  hs::Pool& m = r->pool;
  m.release(&r->d_pf);
  m.release(&r->d_pb);
  m.release(&r->d_part);
  m.release(&r->d_trace);
  r->n = 0;
  r->cap = n;  // planes of exactly n: the [2][n] energy blocks are two adjacent planes
  const size_t nb = (size_t)((n + HS_REF_PPB - 1) / HS_REF_PPB);
  HS_TRY(m.alloc(&r->d_pf, PF_COUNT * (size_t)n));
  HS_TRY(m.alloc(&r->d_pb, 3 * (size_t)n));
  HS_TRY(m.alloc(&r->d_part, HS_REF_NRED * nb));
  if (r->tracing) HS_TRY(m.alloc_zero(&r->d_trace, 16 * nb, r->stream));
  return HS_OK;
}

// level 0 of a device image (include/hs_image.h) as FirstFrame / SecondFrame ->frame->DirPyr[0]: device to device behind
// the image's last set, no host wait (every reader of dst runs on the refiner's stream)
static int set_image(hs_refiner* r, hs_image* im, float4* hs_refiner::*dst, bool hs_refiner::*have,
                     float hs_refiner::*expo, float ab_exposure) {
  if (!r || !im) return hs::fail(HS_ERR_INVALID, "null argument");
  HsImageView v;
  HS_TRY(hs_image_view(im, r->device, r->W, r->H, 1, false, &v));
  HS_HIP(hipSetDevice(r->device));
  HS_HIP(hipStreamWaitEvent(r->stream, v.ready, 0));
  HS_HIP(hipMemcpyAsync(r->*dst, v.lvl[0], sizeof(float4) * (size_t)r->W * r->H, hipMemcpyDeviceToDevice, r->stream));
  HS_HIP(hs_image_consumed(im, r->stream));
  r->*expo = ab_exposure;
  r->*have = true;
  return HS_OK;
}

// the checks hs_refiner_set_points_flow makes of its flow context: its first frame's keys on the device
static int flow_first_points(hs_refiner* r, hs_flow* f, int* n, const float2** d_first) {
  int dev = 0, w = 0, h = 0;
  if (!hs_flow_first_points(f, &dev, &w, &h, n, d_first))
    return hs::fail(HS_ERR_STATE, "the flow holds no first frame (hs_flow_set_first)");
  if (dev != r->device) return hs::fail(HS_ERR_INVALID, "flow and refiner are on different devices");
  if (w != r->W || h != r->H) return hs::fail(HS_ERR_INVALID, "flow size differs from the refiner's");
  if (*n <= 0) return hs::fail(HS_ERR_INVALID, "the flow's first frame has no points");
  return HS_OK;
}

// the ctor's Pnt set-up from device arrays (enqueued on the refiner's stream or complete): keys, Triangulated, Pts3D.z
static int points_from_device(hs_refiner* r, int n, const float2* d_first, const uint8_t* d_tri, const float* d_z) {
  hs::Pool scratch;  // freed on every return path
  int* d_bad = nullptr;
  HS_TRY(scratch.alloc_zero(&d_bad, 1, r->stream));
  HS_TRY(alloc_points(r, n));
  hipStream_t s = r->stream;
  HsRefPointsArgs a;
  a.n = n;
  a.W = r->W;
  a.H = r->H;
  a.n_planes = PF_COUNT;
  a.pl_u = PF_U; a.pl_v = PF_V; a.pl_invz = PF_INVZ; a.pl_id = PF_ID; a.pl_idn = PF_IDN; a.pl_ir = PF_IR;
  a.first = d_first;
  a.tri = d_tri;
  a.z = d_z;
  a.pf = r->d_pf;
  a.pb = r->d_pb;
  a.n_bad = d_bad;
  hipLaunchKernelGGL(hs_k_ref_points, dim3((n + 255) / 256), dim3(256), 0, s, a);
  HS_HIP(hipGetLastError());
  // the one read-back: the keys outside the image (also the wait after which tri / z / the flow's keys are free)
  HS_HIP(hipMemcpyAsync(&r->h_flags[2], d_bad, sizeof(int), hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  if (r->h_flags[2] != 0) return hs::fail(HS_ERR_INVALID, "keypoint outside the image");  // r->n stays 0: no points
  r->n = n;
  r->jb_sel = 0;
  r->last_iters = 0;
  return HS_OK;
}

extern "C" {

int hs_refiner_create(hs_refiner** out, int device_id, int width, int height, const double K4[4]) {
  if (!out || !K4 || width < 8 || height < 8) return hs::fail(HS_ERR_INVALID, "bad refiner arguments");
  *out = nullptr;
  HS_TRY(hs::check_device(device_id));
  hs_refiner* r = new hs_refiner();
  r->W = width;
  r->H = height;
  r->tracing = hs::env::ktrace();
  for (int q = 0; q < 4; q++) r->K4[q] = K4[q];
  const double K[9] = {K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1};
  inv3d(K, r->Ki);
  const size_t np = (size_t)width * height;
  hs::Pool& m = r->pool;
  int rc = HS_OK;
  if (r->open(device_id) || m.alloc(&r->d_img1, np) || m.alloc(&r->d_img2, np) || m.pinned(&r->h_ctl, 1) ||
      m.pinned(&r->h_flags, 4) || m.alloc_zero(&r->d_ticket, 1, r->stream) || m.alloc_zero(&r->d_ctl, 1, r->stream) ||
      m.alloc(&r->d_log, (size_t)HS_REF_MAXLOG * HS_REF_LOGW))
    rc = hs::fail(HS_ERR_HIP, "refiner allocation failed");
  if (rc) hs_refiner_destroy(r);
  else *out = r;
  return rc;
}

void hs_refiner_destroy(hs_refiner* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  if (r->stream) (void)hipStreamSynchronize(r->stream);
  r->pool.release_all();
  if (r->ev_handoff) (void)hipEventDestroy(r->ev_handoff);
  r->close();
  delete r;
}

int hs_refiner_set_frames(hs_refiner* r, const float* first, const float* second, float e1, float e2) {
  if (!r || !first || !second) return hs::fail(HS_ERR_INVALID, "null frame");
  HS_HIP(hipSetDevice(r->device));
  const size_t np = (size_t)r->W * r->H;
  std::vector<float4> tex(np);
  float4* dst[2] = {r->d_img1, r->d_img2};
  const float* src[2] = {first, second};
  for (int f = 0; f < 2; f++) {
    hs::texels_from_triplets(tex.data(), src[f], np);
    HS_HIP(hipMemcpyAsync(dst[f], tex.data(), np * sizeof(float4), hipMemcpyHostToDevice, r->stream));
    HS_HIP(hipStreamSynchronize(r->stream));  // tex is reused
  }
  r->expo1 = e1;
  r->expo2 = e2;
  r->have1 = r->have2 = true;
  return HS_OK;
}

int hs_refiner_set_points(hs_refiner* r, int n, const float* u, const float* v, const uint8_t* tri, const float* z) {
  if (!r || n <= 0 || !u || !v || !tri || !z) return hs::fail(HS_ERR_INVALID, "bad points");
  for (int i = 0; i < n; i++)
    if (!std::isfinite(u[i]) || !std::isfinite(v[i]) || u[i] < 0 || v[i] < 0 || u[i] > r->W - 1 || v[i] > r->H - 1)
      return hs::fail(HS_ERR_INVALID, "keypoint outside the image");
  HS_HIP(hipSetDevice(r->device));
  HS_TRY(alloc_points(r, n));
  // the ctor's Pnt set-up (Src/Initializer.cpp:1362-1382)
  std::vector<float> pf((size_t)PF_COUNT * n, 0.f);
  std::vector<uint8_t> pb(3 * (size_t)n, 0);
  for (int i = 0; i < n; i++) {
    const float invz = tri[i] ? (float)(1.0 / z[i]) : 1.0f;
    pf[PF_U * (size_t)n + i] = u[i];
    pf[PF_V * (size_t)n + i] = v[i];
    pf[PF_INVZ * (size_t)n + i] = invz;
    pf[PF_ID * (size_t)n + i] = invz;
    pf[PF_IDN * (size_t)n + i] = invz;
    pf[PF_IR * (size_t)n + i] = invz;
    pb[i] = tri[i] ? 1 : 0;
    pb[n + i] = 1;  // isGood
  }
  HS_HIP(hipMemcpyAsync(r->d_pf, pf.data(), pf.size() * sizeof(float), hipMemcpyHostToDevice, r->stream));
  HS_HIP(hipMemcpyAsync(r->d_pb, pb.data(), pb.size(), hipMemcpyHostToDevice, r->stream));
  HS_HIP(hipStreamSynchronize(r->stream));
  r->n = n;
  r->jb_sel = 0;
  r->last_iters = 0;
  return HS_OK;
}

int hs_refiner_set_first_image(hs_refiner* r, hs_image* im, float ab_exposure) {
  return set_image(r, im, &hs_refiner::d_img1, &hs_refiner::have1, &hs_refiner::expo1, ab_exposure);
}

int hs_refiner_set_second_image(hs_refiner* r, hs_image* im, float ab_exposure) {
  return set_image(r, im, &hs_refiner::d_img2, &hs_refiner::have2, &hs_refiner::expo2, ab_exposure);
}

int hs_refiner_set_points_flow(hs_refiner* r, hs_flow* f, const uint8_t* tri, const float* z) {
  if (!r || !f || !tri || !z) return hs::fail(HS_ERR_INVALID, "null argument");
  int n = 0;
  const float2* d_first = nullptr;
  HS_TRY(flow_first_points(r, f, &n, &d_first));
  HS_HIP(hipSetDevice(r->device));
  hs::Pool scratch;  // freed on every return path
  uint8_t* d_tri = nullptr;
  float* d_z = nullptr;
  HS_TRY(scratch.alloc(&d_tri, (size_t)n));
  HS_TRY(scratch.alloc(&d_z, (size_t)n));
  HS_HIP(hipMemcpyAsync(d_tri, tri, (size_t)n, hipMemcpyHostToDevice, r->stream));
  HS_HIP(hipMemcpyAsync(d_z, z, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, r->stream));
  return points_from_device(r, n, d_first, d_tri, d_z);
}

int hs_refiner_set_points_twoview(hs_refiner* r, hs_flow* f, hs_twoview* tv) {
  if (!r || !f || !tv) return hs::fail(HS_ERR_INVALID, "null argument");
  int n = 0, tv_dev = 0, tv_n = 0;
  const float2* d_first = nullptr;
  const uint8_t* d_tri = nullptr;
  const float* d_z = nullptr;
  HS_TRY(flow_first_points(r, f, &n, &d_first));
  const bool fresh = hs_twoview_triangulated(tv, f, &tv_dev, &tv_n, &d_tri, &d_z);
  if (tv_dev != r->device) return hs::fail(HS_ERR_INVALID, "two-view fit and refiner are on different devices");
  if (!fresh || tv_n != n)
    return hs::fail(HS_ERR_STATE, "the two-view fit holds no successful fit of this flow's first frame and key count");
  HS_HIP(hipSetDevice(r->device));
  // the fit waited for its kernels before it returned: its arrays are complete, and this call waits for its reads
  return points_from_device(r, n, d_first, d_tri, d_z);
}

int hs_refiner_get_videpth(hs_refiner* r, float* videpth) {
  if (!r || !videpth) return hs::fail(HS_ERR_INVALID, "null");
  if (r->n <= 0) return hs::fail(HS_ERR_STATE, "no points");
  HS_HIP(hipSetDevice(r->device));
  const size_t n = r->n;
  std::vector<float> id(n), iz(n);
  std::vector<uint8_t> tri(n), good(n);
  const HsRefPoints p = points_of(r);
  HS_HIP(hipMemcpyAsync(id.data(), p.idepth, n * sizeof(float), hipMemcpyDeviceToHost, r->stream));
  HS_HIP(hipMemcpyAsync(iz.data(), p.invz, n * sizeof(float), hipMemcpyDeviceToHost, r->stream));
  HS_HIP(hipMemcpyAsync(tri.data(), p.tri, n, hipMemcpyDeviceToHost, r->stream));
  HS_HIP(hipMemcpyAsync(good.data(), p.good, n, hipMemcpyDeviceToHost, r->stream));
  HS_HIP(hipStreamSynchronize(r->stream));
  for (size_t i = 0; i < n; i++) videpth[i] = hs::init_videpth(tri[i] != 0, good[i] != 0, id[i], iz[i]);
  return HS_OK;
}

int hs_refiner_seed_ba(hs_refiner* r, hs_ctx* ba, int frame, uint8_t* why_out, int* handles_out, int* n_seeded) {
  if (!r || !ba) return hs::fail(HS_ERR_INVALID, "null argument");
  if (ba->comm_lost) return hs::fail(HS_ERR_RCCL, "communicator aborted by an earlier call (a peer rank failed)");
  if (ba->multi_rank()) return hs::fail(HS_ERR_STATE, "hs_refiner_seed_ba needs a single-rank BA context");
  if (r->n <= 0) return hs::fail(HS_ERR_STATE, "no points (hs_refiner_set_points / hs_refiner_set_points_flow)");
  if (!r->have1) return hs::fail(HS_ERR_STATE, "no first frame (hs_refiner_set_first_image / hs_refiner_set_frames)");
  if (ba->device != r->device) return hs::fail(HS_ERR_INVALID, "refiner and BA context on different devices");
  if (!ba->d_state || !ba->haveCam) return hs::fail(HS_ERR_STATE, "the BA context has no window");
  if (ba->cam.width != r->W || ba->cam.height != r->H) return hs::fail(HS_ERR_INVALID, "image size mismatch");
  HS_TRY(hs::seed_frame_check(ba, frame));
  HS_HIP(hipSetDevice(r->device));
  const int n = r->n;
  if (n > r->seed_cap) {
    r->seed_cap = 0;
    HS_TRY(r->pool.alloc(&r->d_why, (size_t)n));
    HS_TRY(r->pool.pinned(&r->h_why, (size_t)n));
    if (!r->d_nseed) HS_TRY(r->pool.alloc(&r->d_nseed, 1));
    r->seed_cap = n;
  }
  if (!r->ev_handoff) HS_HIP(hipEventCreateWithFlags(&r->ev_handoff, hipEventDisableTiming));
  hipStream_t s = r->stream;
  // the refiner's stream after the BA's: its last commit gathered from the staging array written here
  HS_HIP(hipEventRecord(ba->ev_ready, ba->stream));
  HS_HIP(hipStreamWaitEvent(s, ba->ev_ready, 0));
  const HsRefPoints p = points_of(r);
  HsInitSeedArgs a;
  a.n = n;
  a.W = r->W;
  a.H = r->H;
  a.base = ba->n_dev_staged;
  a.room = std::max(0, ba->cap_P - ba->n_dev_staged);
  a.img = r->d_img1;
  a.u = p.u;
  a.v = p.v;
  a.invz = p.invz;
  a.idepth = p.idepth;
  a.tri = p.tri;
  a.good = p.good;
  a.outlierTHSumComponent = ba->P.outlierTHSumComponent;
  a.priorF = ba->P.idepthFixPrior * 1.0f * 1.0f;  // as hs_ba_insert_points with has_depth_prior
  a.why = r->d_why;
  a.n_seeded = r->d_nseed;
  a.out = ba->d_act_stage;
  hipLaunchKernelGGL(hs_k_init_seed, dim3(1), dim3(1024), 0, s, a);
  HS_HIP(hipGetLastError());
  // the structural read-back: why (n bytes) and the count; the mirror has to learn how many points joined
  HS_HIP(hipMemcpyAsync(r->h_why, r->d_why, (size_t)n, hipMemcpyDeviceToHost, s));
  HS_HIP(hipMemcpyAsync(&r->h_flags[1], r->d_nseed, sizeof(int), hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  const int ns = r->h_flags[1];
  if (hs::mirror_points(ba) + ns > ba->cap_P || ba->n_dev_staged + ns > ba->cap_P)
    return hs::fail(HS_ERR_NOMEM, "seeded points exceed the BA context's point capacity (hs_ba_reserve)");
  HS_TRY(hs::stage_seeded(ba, ns, frame, handles_out));
  // the BA's commit gathers the staged points: its stream after the refiner's
  HS_HIP(hipEventRecord(r->ev_handoff, s));
  HS_HIP(hipStreamWaitEvent(ba->stream, r->ev_handoff, 0));
  if (why_out) std::memcpy(why_out, r->h_why, (size_t)n);
  if (n_seeded) *n_seeded = ns;
  return HS_OK;
}

int hs_refiner_refine(hs_refiner* r, double pose[7], float* idepth_out, uint8_t* good_out, int* iterations,
                      int* snapped) {
  if (!r || !pose) return hs::fail(HS_ERR_INVALID, "null");
  double aff[2] = {0, 0};  // thisToNext_aff = AffLight(0, 0)
  if (r->expo1 > 0 && r->expo2 > 0) aff[0] = (double)logf(r->expo2 / r->expo1);
  HS_TRY(run_refine(r, pose, aff));
  const HsRefCtl& o = *r->h_ctl;
  for (int q = 0; q < 7; q++) pose[q] = o.T[q];
  if (iterations) *iterations = r->last_iters;
  if (snapped) *snapped = o.snapped;
  if (idepth_out || good_out) {
    const size_t n = r->n;
    std::vector<float> id(n);
    std::vector<uint8_t> tri(n), good(n);
    const HsRefPoints p = points_of(r);
    HS_HIP(hipMemcpyAsync(id.data(), p.idepth, n * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    HS_HIP(hipMemcpyAsync(tri.data(), p.tri, n, hipMemcpyDeviceToHost, r->stream));
    HS_HIP(hipMemcpyAsync(good.data(), p.good, n, hipMemcpyDeviceToHost, r->stream));
    HS_HIP(hipStreamSynchronize(r->stream));
    for (size_t i = 0; i < n; i++) {
      if (good_out) good_out[i] = good[i];
      if (idepth_out && good[i] && tri[i]) idepth_out[i] = id[i];  // _videpth write-back (:1389-1395)
    }
  }
  if (!std::isfinite(o.resOld[0])) return hs::fail(HS_ERR_NONFINITE, "non-finite refinement energy");
  return HS_OK;
}

int hs_refiner_calc_res(hs_refiner* r, const double T7[7], const double aff[2], float* H64, float* b8, float* Hsc64,
                        float* bsc8, float res3[3]) {
  if (!r || !T7 || !aff) return hs::fail(HS_ERR_INVALID, "null");
  HS_TRY(run_calc(r, T7, aff));
  const HsRefCtl& o = *r->h_ctl;
  if (H64) std::memcpy(H64, o.H, sizeof(o.H));
  if (b8) std::memcpy(b8, o.b, sizeof(o.b));
  if (Hsc64) std::memcpy(Hsc64, o.Hsc, sizeof(o.Hsc));
  if (bsc8) std::memcpy(bsc8, o.bsc, sizeof(o.bsc));
  if (res3) std::memcpy(res3, o.res, sizeof(o.res));
  return HS_OK;
}

int hs_refiner_get_points(hs_refiner* r, float* f7, uint8_t* g2, float* jb_new) {
  if (!r || !f7 || !g2) return hs::fail(HS_ERR_INVALID, "null");
  if (r->n <= 0) return hs::fail(HS_ERR_STATE, "no points");
  HS_HIP(hipSetDevice(r->device));
  const size_t n = r->n;
  std::vector<float> pf((size_t)PF_COUNT * n);
  std::vector<uint8_t> pb(3 * n);
  HS_HIP(hipMemcpyAsync(pf.data(), r->d_pf, pf.size() * sizeof(float), hipMemcpyDeviceToHost, r->stream));
  HS_HIP(hipMemcpyAsync(pb.data(), r->d_pb, pb.size(), hipMemcpyDeviceToHost, r->stream));
  HS_HIP(hipStreamSynchronize(r->stream));
  const int planes[7] = {PF_ID, PF_IDN, PF_IR, PF_EN0, PF_EN1, PF_MS, PF_LHN};
  for (size_t i = 0; i < n; i++) {
    for (int k = 0; k < 7; k++) f7[7 * i + k] = pf[planes[k] * n + i];
    g2[2 * i] = pb[n + i];
    g2[2 * i + 1] = pb[2 * n + i];
  }
  if (jb_new) {  // JbBuffer_new = the plane the next calcResAndGS writes
    const int base = PF_JB0 + 10 * (r->jb_sel ^ 1);
    for (size_t i = 0; i < n; i++)
      for (int k = 0; k < 10; k++) jb_new[10 * i + k] = pf[(base + k) * n + i];
  }
  return HS_OK;
}

int hs_refiner_get_log(hs_refiner* r, int cap, float* out) {
  if (!r || (cap > 0 && !out)) return hs::fail(HS_ERR_INVALID, "null");
  const int n = std::min(r->last_iters, HS_REF_MAXLOG);
  const int m = std::min(n, cap);
  if (m > 0) {
    HS_HIP(hipSetDevice(r->device));
    HS_HIP(hipStreamSynchronize(r->stream));
    HS_HIP(hipMemcpy(out, r->d_log, sizeof(float) * HS_REF_LOGW * m, hipMemcpyDeviceToHost));
  }
  return n;
}

int hs_refiner_last_ms(hs_refiner* r, double* ms) {
  if (!r || !ms) return hs::fail(HS_ERR_INVALID, "null");
  *ms = r->last_ms;
  return HS_OK;
}

}  // extern "C"
