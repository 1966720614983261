// hs_twoview.cpp — the two-view fit context of include/hs_twoview.h: argument checks, the fit's buffers (all taken at
// create) and the chain of launches of hs_twoview_kernels.hip on the context's stream, with one wait per call.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/hs_twoview.h"
#include "hs_flow_kernels.h"
#include "hs_host.h"
#include "hs_twoview_kernels.h"

static_assert(sizeof(hs_twoview_result) == 128, "hs_twoview_result is 128 bytes (hslam_amd/twoview.py mirrors it)");

constexpr int kTvStages = 8;

struct hs_twoview : hs::Device {
  hs::Pool pool;
  int cap = 0;
  float K[4] = {0, 0, 0, 0};
  HsTvState* d_st = nullptr;
  HsTvState* h_st = nullptr;  // pinned
  // a host-fed fit's inputs
  float2 *d_in1 = nullptr, *d_in2 = nullptr;
  uint8_t* d_in_status = nullptr;
  int* d_in_sets = nullptr;
  int* h_sets = nullptr;  // pinned
  // the state
  float4* d_keys = nullptr;
  uint8_t* d_status = nullptr;
  int* d_sets = nullptr;
  float *d_norm = nullptr, *d_models = nullptr, *d_h12 = nullptr, *d_scores = nullptr;
  uint8_t* d_inl = nullptr;
  float *d_rt_p3d = nullptr, *d_rt_cos = nullptr;
  uint8_t *d_rt_pass = nullptr, *d_rt_good = nullptr;
  uint8_t* d_tri = nullptr;
  float *d_z = nullptr, *d_p3d = nullptr;
  hipEvent_t ev_flow = nullptr;           // orders a fit behind the flow's last track
  hipEvent_t ev_k[kTvStages + 1] = {};    // between the kernels of a fit
  hipEvent_t ev_d[3] = {};                // around the two kernels of a draw
  // the draw of the sets: the generator's state (randomGen) is the host's, its words go up, m comes back
  uint64_t rng = 0;
  int* d_all = nullptr;
  uint32_t* d_words = nullptr;
  uint32_t* h_words = nullptr;  // pinned
  int* h_draw = nullptr;        // pinned: hs_twoview_draw's sets and m
  int n_sets_fit = 0;           // the sets of the last fit at d_sets
  bool drew = false;
  int n = 0, ns_h = 0, ns_f = 0, n_rt = 0;
  bool have_keys = false, have_fit = false, fit_ok = false, timed = false;
  hs_flow* fit_flow = nullptr;            // the flow of the last fit (null: host-fed), identified by
  long long fit_first_id = -1;            // its first frame
  hs_twoview_result last = {};
};

namespace {

inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }

HsTvArgs args_of(hs_twoview* tv, int n, int ns_h, int ns_f) {
  HsTvArgs a;
  std::memset(&a, 0, sizeof a);
  a.n = n;
  a.ns_h = ns_h;
  a.ns_f = ns_f;
  a.fx = tv->K[0];
  a.fy = tv->K[1];
  a.cx = tv->K[2];
  a.cy = tv->K[3];
  a.st = tv->d_st;
  a.in1 = tv->d_in1;
  a.in2 = tv->d_in2;
  a.in_status = tv->d_in_status;
  a.in_sets = tv->d_in_sets;
  a.keys = tv->d_keys;
  a.status = tv->d_status;
  a.sets = tv->d_sets;
  a.norm = tv->d_norm;
  a.models = tv->d_models;
  a.h12 = tv->d_h12;
  a.scores = tv->d_scores;
  a.inl = tv->d_inl;
  a.rt_p3d = tv->d_rt_p3d;
  a.rt_cos = tv->d_rt_cos;
  a.rt_pass = tv->d_rt_pass;
  a.rt_good = tv->d_rt_good;
  a.tri = tv->d_tri;
  a.z = tv->d_z;
  a.p3d = tv->d_p3d;
  a.all = tv->d_all;
  a.words = tv->d_words;
  a.draw_out = tv->d_sets;
  return a;
}

// the sets' host rules: the count, the range, the distinct indices; with `status` also the status rule
int check_sets(int n, int n_sets, const int32_t* sets, const uint8_t* status) {
  if (!sets) return hs::fail(HS_ERR_INVALID, "null sets");
  if (n_sets < 1 || n_sets > kTvMaxSets)
    return hs::fail(HS_ERR_INVALID, "n_sets is " + std::to_string(n_sets) + ", must be 1 .. 256");
  for (int s = 0; s < n_sets; s++)
    for (int j = 0; j < 8; j++) {
      const int idx = sets[s * 8 + j];
      if (idx < 0 || idx >= n)
        return hs::fail(HS_ERR_INVALID, "set " + std::to_string(s) + " holds index " + std::to_string(idx) +
                                            ", out of range for " + std::to_string(n) + " keys");
      if (status && !status[idx])
        return hs::fail(HS_ERR_INVALID, "set " + std::to_string(s) + " points at key " + std::to_string(idx) +
                                            " with status 0");
      for (int k = 0; k < j; k++)
        if (sets[s * 8 + k] == idx)
          return hs::fail(HS_ERR_INVALID, "set " + std::to_string(s) + " repeats index " + std::to_string(idx));
    }
  return HS_OK;
}

// cv::RNG (the contract of include/hs_twoview.h)
inline uint64_t rng_seeded(uint64_t seed) { return seed ? seed : 0xffffffffull; }
inline uint32_t rng_next(uint64_t* state) {
  *state = (uint64_t)(uint32_t)*state * 4164903690u + (uint32_t)(*state >> 32);
  return (uint32_t)*state;
}

int check_n_sets(int n_sets) {
  if (n_sets < 1 || n_sets > kTvMaxSets)
    return hs::fail(HS_ERR_INVALID, "n_sets is " + std::to_string(n_sets) + ", must be 1 .. 256");
  return HS_OK;
}

// The words of a draw of n_sets sets from tv's state, uploaded on the stream; after[0] / after[1] = the state behind
// 7 / 8 words per set (m == 8 takes 7).  The context's state is not moved.
int upload_words(hs_twoview* tv, int n_sets, uint64_t after[2]) {
  uint64_t st = tv->rng;
  for (int i = 0; i < 8 * n_sets; i++) {
    if (i == 7 * n_sets) after[0] = st;
    tv->h_words[i] = rng_next(&st);
  }
  after[1] = st;
  HS_HIP(hipMemcpyAsync(tv->d_words, tv->h_words, sizeof(uint32_t) * 8 * (size_t)n_sets, hipMemcpyHostToDevice,
                        tv->stream));
  return HS_OK;
}

#define HS_TV_LAUNCH(kernel, grid, block, stage)                      \
  do {                                                                \
    hipLaunchKernelGGL(kernel, grid, dim3(block), 0, s, a);           \
    HS_HIP(hipGetLastError());                                        \
    if ((stage) >= 0) HS_HIP(hipEventRecord(tv->ev_k[(stage) + 1], s)); \
  } while (0)

// the launches of one fit behind its inputs; `a` names where the inputs are
// (a.n_draw != 0: the sets are drawn first, from the words upload_words left, and `after` holds the two candidate states)
int run_fit(hs_twoview* tv, HsTvArgs a, hs_flow* flow, long long first_id, hs_twoview_result* result,
            const uint64_t* after = nullptr) {
  hipStream_t s = tv->stream;
  const int n = a.n, ns = a.ns_h;
  HS_TV_LAUNCH(hs_k_tv_begin, dim3(1), 256, -1);
  if (a.n_draw) {
    HS_HIP(hipEventRecord(tv->ev_d[0], s));
    HS_TV_LAUNCH(hs_k_tv_good_list, dim3(1), 1024, -1);
    HS_HIP(hipEventRecord(tv->ev_d[1], s));
    HS_TV_LAUNCH(hs_k_tv_draw, dim3((a.n_draw + 63) / 64), 64, -1);
    HS_HIP(hipEventRecord(tv->ev_d[2], s));
  }
  HS_TV_LAUNCH(hs_k_tv_pack, dim3(blocks((size_t)(n > ns * 8 ? n : ns * 8))), 256, -1);
  HS_HIP(hipEventRecord(tv->ev_k[0], s));
  HS_TV_LAUNCH(hs_k_tv_normalize, dim3(2), 256, 0);
  HS_TV_LAUNCH(hs_k_tv_hypotheses, dim3(2 * ns), 64, 1);  // one wave per (set, model)
  HS_TV_LAUNCH(hs_k_tv_scores, dim3(2 * ns), 256, 2);
  HS_TV_LAUNCH(hs_k_tv_winners, dim3(blocks(n)), 256, 3);
  HS_TV_LAUNCH(hs_k_tv_decompose, dim3(1), 64, 4);
  HS_TV_LAUNCH(hs_k_tv_check_rt, dim3(blocks(n), kTvMaxRt), 256, 5);
  HS_TV_LAUNCH(hs_k_tv_select, dim3(kTvMaxRt), 256, 6);
  HS_TV_LAUNCH(hs_k_tv_finish, dim3(1), 256, 7);
  // the one read-back: the result record (with the status rule's verdict)
  HS_HIP(hipMemcpyAsync(tv->h_st, tv->d_st, sizeof(HsTvState), hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  if (a.n_draw) tv->drew = true;
  if (tv->h_st->bad == 2) {
    // fewer than 8 matched keys: no kernel of the fit ran, the state does not move
    hs_twoview_result r;
    std::memset(&r, 0, sizeof r);
    r.why = 5;
    r.model = r.best_h = r.best_f = r.best_rt = -1;
    r.reserved[0] = (int32_t)(uint32_t)tv->rng;
    r.reserved[1] = (int32_t)(uint32_t)(tv->rng >> 32);
    tv->have_fit = tv->timed = true;
    tv->fit_ok = false;
    tv->last = r;
    if (result) *result = r;
    return HS_OK;
  }
  if (tv->h_st->bad) return hs::fail(HS_ERR_INVALID, "a set points at a key with status 0");
  if (a.n_draw) {
    tv->rng = after[tv->h_st->m == 8 ? 0 : 1];
    tv->h_st->res.reserved[0] = (int32_t)(uint32_t)tv->rng;
    tv->h_st->res.reserved[1] = (int32_t)(uint32_t)(tv->rng >> 32);
  }
  tv->n_sets_fit = ns;
  tv->n = n;
  tv->ns_h = tv->ns_f = ns;
  tv->n_rt = tv->h_st->n_rt;
  tv->have_keys = tv->have_fit = tv->timed = true;
  tv->last = tv->h_st->res;
  tv->fit_ok = tv->last.ok != 0;
  tv->fit_flow = flow;
  tv->fit_first_id = first_id;
  if (result) *result = tv->last;
  return HS_OK;
}

int need_keys(const hs_twoview* tv) {
  if (!tv->have_keys) return hs::fail(HS_ERR_STATE, "no fit yet: hs_twoview_fit / hs_twoview_fit_flow first");
  return HS_OK;
}

}  // namespace

bool hs_twoview_triangulated(hs_twoview* tv, hs_flow* flow, int* device, int* n, const uint8_t** d_tri,
                             const float** d_z) {
  *device = tv->device;
  *n = tv->n;
  *d_tri = tv->d_tri;
  *d_z = tv->d_z;
  if (!tv->have_fit || !tv->fit_ok || tv->fit_flow != flow) return false;
  HsFlowKeys k;
  if (!hs_flow_tracked_keys(flow, &k)) return false;
  return k.first_id == tv->fit_first_id && k.n == tv->n;
}

extern "C" {

int hs_twoview_create(hs_twoview** out, int device_id, int capacity, const double K4[4]) {
  if (!out || !K4) return hs::fail(HS_ERR_INVALID, "null argument");
  *out = nullptr;
  if (capacity < 8) return hs::fail(HS_ERR_INVALID, "capacity must be >= 8: a set takes 8 keys");
  if (capacity > (1 << 24)) return hs::fail(HS_ERR_INVALID, "capacity too large");
  HS_TRY(hs::check_device(device_id));
  hs_twoview* tv = new hs_twoview();
  tv->cap = capacity;
  for (int q = 0; q < 4; q++) tv->K[q] = (float)K4[q];
  const size_t c = capacity;
  int rc = [&]() -> int {
    hs::Pool& m = tv->pool;
    HS_TRY(tv->open(device_id));
    hipStream_t s = tv->stream;
    HS_HIP(hipEventCreateWithFlags(&tv->ev_flow, hipEventDisableTiming));
    for (hipEvent_t& e : tv->ev_k) HS_HIP(hipEventCreate(&e));
    for (hipEvent_t& e : tv->ev_d) HS_HIP(hipEventCreate(&e));
    HS_TRY(m.alloc_zero(&tv->d_st, 1, s));
    HS_TRY(m.pinned(&tv->h_st, 1));
    HS_TRY(m.pinned(&tv->h_sets, (size_t)kTvMaxSets * 8));
    HS_TRY(m.alloc(&tv->d_in1, c));
    HS_TRY(m.alloc(&tv->d_in2, c));
    HS_TRY(m.alloc(&tv->d_in_status, c));
    HS_TRY(m.alloc(&tv->d_in_sets, (size_t)kTvMaxSets * 8));
    // every read-back may come before the kernel that fills its buffer has run (a refused first fit)
    HS_TRY(m.alloc_zero(&tv->d_keys, c, s));
    HS_TRY(m.alloc_zero(&tv->d_status, c, s));
    HS_TRY(m.alloc_zero(&tv->d_sets, (size_t)kTvMaxSets * 8, s));
    HS_TRY(m.alloc_zero(&tv->d_norm, 8, s));
    HS_TRY(m.alloc_zero(&tv->d_models, (size_t)2 * kTvMaxSets * 9, s));
    HS_TRY(m.alloc_zero(&tv->d_h12, (size_t)kTvMaxSets * 9, s));
    HS_TRY(m.alloc_zero(&tv->d_scores, (size_t)2 * kTvMaxSets, s));
    HS_TRY(m.alloc_zero(&tv->d_inl, 2 * c, s));
    HS_TRY(m.alloc_zero(&tv->d_rt_p3d, (size_t)kTvMaxRt * c * 3, s));
    HS_TRY(m.alloc_zero(&tv->d_rt_cos, (size_t)kTvMaxRt * c, s));
    HS_TRY(m.alloc_zero(&tv->d_rt_pass, (size_t)kTvMaxRt * c, s));
    HS_TRY(m.alloc_zero(&tv->d_rt_good, (size_t)kTvMaxRt * c, s));
    HS_TRY(m.alloc_zero(&tv->d_tri, c, s));
    HS_TRY(m.alloc_zero(&tv->d_z, c, s));
    HS_TRY(m.alloc_zero(&tv->d_p3d, 3 * c, s));
    HS_TRY(m.alloc_zero(&tv->d_all, c, s));
    HS_TRY(m.alloc_zero(&tv->d_words, (size_t)kTvMaxSets * 8, s));
    HS_TRY(m.pinned(&tv->h_words, (size_t)kTvMaxSets * 8));
    HS_TRY(m.pinned(&tv->h_draw, (size_t)kTvMaxSets * 8 + 1));
    tv->rng = rng_seeded(0);
    HS_HIP(hipStreamSynchronize(s));
    return HS_OK;
  }();
  if (rc) hs_twoview_destroy(tv);
  else *out = tv;
  return rc;
}

void hs_twoview_destroy(hs_twoview* tv) {
  if (!tv) return;
  (void)hipSetDevice(tv->device);
  if (tv->stream) (void)hipStreamSynchronize(tv->stream);
  tv->pool.release_all();
  if (tv->ev_flow) (void)hipEventDestroy(tv->ev_flow);
  for (hipEvent_t e : tv->ev_k)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : tv->ev_d)
    if (e) (void)hipEventDestroy(e);
  tv->close();
  delete tv;
}

int hs_twoview_fit(hs_twoview* tv, int n, const float* xy1, const float* xy2, const uint8_t* status, int n_sets,
                   const int32_t* sets, hs_twoview_result* result) {
  if (!tv || !xy1 || !xy2 || !status) return hs::fail(HS_ERR_INVALID, "null argument");
  if (n < 8 || n > tv->cap)
    return hs::fail(HS_ERR_INVALID, std::to_string(n) + " keys, must be 8 .. the capacity " + std::to_string(tv->cap));
  HS_TRY(check_sets(n, n_sets, sets, status));
  HS_HIP(hipSetDevice(tv->device));
  hipStream_t s = tv->stream;
  std::memcpy(tv->h_sets, sets, sizeof(int) * 8 * (size_t)n_sets);
  HS_HIP(hipMemcpyAsync(tv->d_in_sets, tv->h_sets, sizeof(int) * 8 * (size_t)n_sets, hipMemcpyHostToDevice, s));
  HS_HIP(hipMemcpyAsync(tv->d_in1, xy1, sizeof(float2) * (size_t)n, hipMemcpyHostToDevice, s));
  HS_HIP(hipMemcpyAsync(tv->d_in2, xy2, sizeof(float2) * (size_t)n, hipMemcpyHostToDevice, s));
  HS_HIP(hipMemcpyAsync(tv->d_in_status, status, (size_t)n, hipMemcpyHostToDevice, s));
  HsTvArgs a = args_of(tv, n, n_sets, n_sets);
  a.n_in_sets = n_sets;
  return run_fit(tv, a, nullptr, -1, result);
}

int hs_twoview_fit_flow(hs_twoview* tv, hs_flow* flow, int n_sets, const int32_t* sets, hs_twoview_result* result) {
  if (!tv || !flow) return hs::fail(HS_ERR_INVALID, "null argument");
  HsFlowKeys k;
  if (!hs_flow_tracked_keys(flow, &k) || !k.tracked)
    return hs::fail(HS_ERR_STATE, "the flow has not tracked a frame yet (hs_flow_set_first, hs_flow_track)");
  if (k.device != tv->device) return hs::fail(HS_ERR_INVALID, "flow and two-view fit are on different devices");
  if (k.n < 8 || k.n > tv->cap)
    return hs::fail(HS_ERR_INVALID, "the flow holds " + std::to_string(k.n) + " keys, must be 8 .. the capacity " +
                                        std::to_string(tv->cap));
  HS_TRY(check_sets(k.n, n_sets, sets, nullptr));
  HS_HIP(hipSetDevice(tv->device));
  hipStream_t s = tv->stream;
  std::memcpy(tv->h_sets, sets, sizeof(int) * 8 * (size_t)n_sets);
  HS_HIP(hipMemcpyAsync(tv->d_in_sets, tv->h_sets, sizeof(int) * 8 * (size_t)n_sets, hipMemcpyHostToDevice, s));
  // behind the flow's last track, without a host wait
  HS_HIP(hipEventRecord(tv->ev_flow, k.stream));
  HS_HIP(hipStreamWaitEvent(s, tv->ev_flow, 0));
  HsTvArgs a = args_of(tv, k.n, n_sets, n_sets);
  a.n_in_sets = n_sets;
  a.in1 = k.first;
  a.in2 = k.matched;
  a.in_status = k.good;
  return run_fit(tv, a, flow, k.first_id, result);  // waits: the flow's arrays are free again on return
}

int hs_twoview_rng_seed(hs_twoview* tv, uint64_t seed) {
  if (!tv) return hs::fail(HS_ERR_INVALID, "null two-view fit");
  tv->rng = rng_seeded(seed);
  return HS_OK;
}

int hs_twoview_rng_skip(hs_twoview* tv, uint64_t n_next) {
  if (!tv) return hs::fail(HS_ERR_INVALID, "null two-view fit");
  if (n_next > (1ull << 30)) return hs::fail(HS_ERR_INVALID, "n_next above 2^30: a skip is a host loop");
  for (uint64_t i = 0; i < n_next; i++) rng_next(&tv->rng);
  return HS_OK;
}

int hs_twoview_rng_state(hs_twoview* tv, uint64_t* state) {
  if (!tv || !state) return hs::fail(HS_ERR_INVALID, "null argument");
  *state = tv->rng;
  return HS_OK;
}

int hs_twoview_draw(hs_twoview* tv, int n, const uint8_t* status, int n_sets, int32_t* sets_out, int* m_out) {
  if (!tv || !status || !sets_out) return hs::fail(HS_ERR_INVALID, "null argument");
  if (n < 8 || n > tv->cap)
    return hs::fail(HS_ERR_INVALID, std::to_string(n) + " keys, must be 8 .. the capacity " + std::to_string(tv->cap));
  HS_TRY(check_n_sets(n_sets));
  int good = 0;
  for (int i = 0; i < n; i++) good += status[i] != 0;
  if (good < 8)
    return hs::fail(HS_ERR_INVALID, std::to_string(good) + " keys with status != 0: a set takes 8");
  HS_HIP(hipSetDevice(tv->device));
  hipStream_t s = tv->stream;
  uint64_t after[2];
  HS_TRY(upload_words(tv, n_sets, after));
  HS_HIP(hipMemcpyAsync(tv->d_in_status, status, (size_t)n, hipMemcpyHostToDevice, s));
  // the fit's own sets stay where hs_twoview_get_sets reads them: the draw lands in the host-fed fit's input buffer
  HsTvArgs a = args_of(tv, n, 0, 0);
  a.n_draw = n_sets;
  a.draw_out = tv->d_in_sets;
  HS_HIP(hipEventRecord(tv->ev_d[0], s));
  HS_TV_LAUNCH(hs_k_tv_good_list, dim3(1), 1024, -1);
  HS_HIP(hipEventRecord(tv->ev_d[1], s));
  HS_TV_LAUNCH(hs_k_tv_draw, dim3((n_sets + 63) / 64), 64, -1);
  HS_HIP(hipEventRecord(tv->ev_d[2], s));
  const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
  HS_HIP(hipMemcpyAsync(tv->h_draw, tv->d_in_sets, sizeof(int) * 8 * (size_t)n_sets, d2h, s));
  HS_HIP(hipMemcpyAsync(tv->h_draw + 8 * (size_t)n_sets, &tv->d_st->m, sizeof(int), d2h, s));
  HS_HIP(hipStreamSynchronize(s));
  const int m = tv->h_draw[8 * (size_t)n_sets];
  std::memcpy(sets_out, tv->h_draw, sizeof(int) * 8 * (size_t)n_sets);
  if (m_out) *m_out = m;
  tv->rng = after[m == 8 ? 0 : 1];
  tv->drew = true;
  return HS_OK;
}

int hs_twoview_fit_flow_drawn(hs_twoview* tv, hs_flow* flow, int n_sets, hs_twoview_result* result) {
  if (!tv || !flow) return hs::fail(HS_ERR_INVALID, "null argument");
  HsFlowKeys k;
  if (!hs_flow_tracked_keys(flow, &k) || !k.tracked)
    return hs::fail(HS_ERR_STATE, "the flow has not tracked a frame yet (hs_flow_set_first, hs_flow_track)");
  if (k.device != tv->device) return hs::fail(HS_ERR_INVALID, "flow and two-view fit are on different devices");
  if (k.n < 8 || k.n > tv->cap)
    return hs::fail(HS_ERR_INVALID, "the flow holds " + std::to_string(k.n) + " keys, must be 8 .. the capacity " +
                                        std::to_string(tv->cap));
  HS_TRY(check_n_sets(n_sets));
  HS_HIP(hipSetDevice(tv->device));
  hipStream_t s = tv->stream;
  uint64_t after[2];
  HS_TRY(upload_words(tv, n_sets, after));
  HS_HIP(hipEventRecord(tv->ev_flow, k.stream));
  HS_HIP(hipStreamWaitEvent(s, tv->ev_flow, 0));
  HsTvArgs a = args_of(tv, k.n, n_sets, n_sets);
  a.n_draw = n_sets;
  a.in1 = k.first;
  a.in2 = k.matched;
  a.in_status = k.good;
  return run_fit(tv, a, flow, k.first_id, result, after);  // waits: the flow's arrays are free again on return
}

int hs_twoview_get_sets(hs_twoview* tv, int32_t* sets) {
  if (!tv || !sets) return hs::fail(HS_ERR_INVALID, "null argument");
  HS_TRY(need_keys(tv));
  HS_HIP(hipSetDevice(tv->device));
  HS_HIP(hipMemcpyAsync(sets, tv->d_sets, sizeof(int) * 8 * (size_t)tv->n_sets_fit, hipMemcpyDeviceToHost, tv->stream));
  HS_HIP(hipStreamSynchronize(tv->stream));
  return HS_OK;
}

int hs_twoview_last_draw_stats(hs_twoview* tv, double* ms) {
  if (!tv || !ms) return hs::fail(HS_ERR_INVALID, "null argument");
  if (!tv->drew) return hs::fail(HS_ERR_STATE, "no draw yet");
  HS_HIP(hipSetDevice(tv->device));
  for (int k = 0; k < 2; k++) {
    float t = 0;
    HS_HIP(hipEventElapsedTime(&t, tv->ev_d[k], tv->ev_d[k + 1]));
    ms[k] = t;
  }
  return HS_OK;
}

int hs_twoview_get(hs_twoview* tv, uint8_t* inliers_h, uint8_t* inliers_f, float* scores_h, float* scores_f,
                   uint8_t* triangulated, float* p3d, float* models) {
  if (!tv) return hs::fail(HS_ERR_INVALID, "null two-view fit");
  HS_TRY(need_keys(tv));
  HS_HIP(hipSetDevice(tv->device));
  hipStream_t s = tv->stream;
  const size_t n = tv->n;
  const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
  if (inliers_h) HS_HIP(hipMemcpyAsync(inliers_h, tv->d_inl, n, d2h, s));
  if (inliers_f) HS_HIP(hipMemcpyAsync(inliers_f, tv->d_inl + n, n, d2h, s));
  if (scores_h) HS_HIP(hipMemcpyAsync(scores_h, tv->d_scores, sizeof(float) * tv->ns_h, d2h, s));
  if (scores_f) HS_HIP(hipMemcpyAsync(scores_f, tv->d_scores + kTvMaxSets, sizeof(float) * tv->ns_f, d2h, s));
  if (triangulated) HS_HIP(hipMemcpyAsync(triangulated, tv->d_tri, n, d2h, s));
  if (p3d) HS_HIP(hipMemcpyAsync(p3d, tv->d_p3d, sizeof(float) * 3 * n, d2h, s));
  if (models) {
    // the library keeps the two halves kTvMaxSets apart; the caller's array is dense (it assumes ns_h == ns_f sets)
    HS_HIP(hipMemcpyAsync(models, tv->d_models, sizeof(float) * 9 * tv->ns_h, d2h, s));
    HS_HIP(hipMemcpyAsync(models + 9 * (size_t)tv->ns_h, tv->d_models + 9 * (size_t)kTvMaxSets,
                          sizeof(float) * 9 * tv->ns_f, d2h, s));
  }
  HS_HIP(hipStreamSynchronize(s));
  return HS_OK;
}

int hs_twoview_last_result(hs_twoview* tv, hs_twoview_result* result) {
  if (!tv || !result) return hs::fail(HS_ERR_INVALID, "null argument");
  if (!tv->have_fit) return hs::fail(HS_ERR_STATE, "no fit yet");
  *result = tv->last;
  return HS_OK;
}

int hs_twoview_get_rt(hs_twoview* tv, int* n_rt, int32_t* n_good, float* parallax, uint8_t* good, uint8_t* pass,
                      float* cos_parallax, float* p3d) {
  if (!tv) return hs::fail(HS_ERR_INVALID, "null two-view fit");
  HS_TRY(need_keys(tv));
  HS_HIP(hipSetDevice(tv->device));
  hipStream_t s = tv->stream;
  if (n_rt) *n_rt = tv->n_rt;
  const size_t m = (size_t)tv->n_rt * tv->n;
  const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
  if (tv->n_rt) {
    if (n_good) HS_HIP(hipMemcpyAsync(n_good, tv->d_st->n_good, sizeof(int) * tv->n_rt, d2h, s));
    if (parallax) HS_HIP(hipMemcpyAsync(parallax, tv->d_st->parallax, sizeof(float) * tv->n_rt, d2h, s));
    if (good) HS_HIP(hipMemcpyAsync(good, tv->d_rt_good, m, d2h, s));
    if (pass) HS_HIP(hipMemcpyAsync(pass, tv->d_rt_pass, m, d2h, s));
    if (cos_parallax) HS_HIP(hipMemcpyAsync(cos_parallax, tv->d_rt_cos, sizeof(float) * m, d2h, s));
    if (p3d) HS_HIP(hipMemcpyAsync(p3d, tv->d_rt_p3d, sizeof(float) * 3 * m, d2h, s));
  }
  HS_HIP(hipStreamSynchronize(s));
  return HS_OK;
}

int hs_twoview_last_stats(hs_twoview* tv, double* ms) {
  if (!tv || !ms) return hs::fail(HS_ERR_INVALID, "null argument");
  if (!tv->timed) return hs::fail(HS_ERR_STATE, "no fit yet");
  HS_HIP(hipSetDevice(tv->device));
  for (int k = 0; k < kTvStages; k++) {
    float t = 0;
    HS_HIP(hipEventElapsedTime(&t, tv->ev_k[k], tv->ev_k[k + 1]));
    ms[k] = t;
  }
  return HS_OK;
}

int hs_twoview_score_models(hs_twoview* tv, int n_h, const float* H21, const float* H12, int n_f, const float* F21) {
  if (!tv || !H21 || !H12 || !F21) return hs::fail(HS_ERR_INVALID, "null argument");
  if (n_h < 1 || n_h > kTvMaxSets || n_f < 1 || n_f > kTvMaxSets)
    return hs::fail(HS_ERR_INVALID, "n_h and n_f must be 1 .. 256");
  HS_TRY(need_keys(tv));
  HS_HIP(hipSetDevice(tv->device));
  hipStream_t s = tv->stream;
  const hipMemcpyKind h2d = hipMemcpyHostToDevice;
  HS_HIP(hipMemcpyAsync(tv->d_models, H21, sizeof(float) * 9 * n_h, h2d, s));
  HS_HIP(hipMemcpyAsync(tv->d_h12, H12, sizeof(float) * 9 * n_h, h2d, s));
  HS_HIP(hipMemcpyAsync(tv->d_models + 9 * (size_t)kTvMaxSets, F21, sizeof(float) * 9 * n_f, h2d, s));
  tv->fit_ok = false;
  tv->ns_h = n_h;
  tv->ns_f = n_f;
  HsTvArgs a = args_of(tv, tv->n, n_h, n_f);
  HS_TV_LAUNCH(hs_k_tv_begin, dim3(1), 256, -1);
  HS_TV_LAUNCH(hs_k_tv_scores, dim3(n_h + n_f), 256, -1);
  HS_TV_LAUNCH(hs_k_tv_winners, dim3(blocks(tv->n)), 256, -1);
  HS_HIP(hipStreamSynchronize(s));
  return HS_OK;
}

int hs_twoview_check_rt(hs_twoview* tv, int n_rt, const float* R, const float* t, const uint8_t* inliers) {
  if (!tv || !R || !t || !inliers) return hs::fail(HS_ERR_INVALID, "null argument");
  if (n_rt < 1 || n_rt > kTvMaxRt) return hs::fail(HS_ERR_INVALID, "n_rt must be 1 .. 8");
  HS_TRY(need_keys(tv));
  HS_HIP(hipSetDevice(tv->device));
  hipStream_t s = tv->stream;
  HsTvState* h = tv->h_st;
  for (int k = 0; k < n_rt; k++) {
    for (int i = 0; i < 9; i++) h->rt[k][i] = R[9 * k + i];
    for (int i = 0; i < 3; i++) h->rt[k][9 + i] = t[3 * k + i];
  }
  h->n_rt = n_rt;
  const hipMemcpyKind h2d = hipMemcpyHostToDevice;
  HS_HIP(hipMemcpyAsync(&tv->d_st->rt[0][0], &h->rt[0][0], sizeof(float) * 12 * n_rt, h2d, s));
  HS_HIP(hipMemcpyAsync(&tv->d_st->n_rt, &h->n_rt, sizeof(int), h2d, s));
  HS_HIP(hipMemcpyAsync(tv->d_in_status, inliers, (size_t)tv->n, h2d, s));
  tv->fit_ok = false;
  tv->n_rt = n_rt;
  HsTvArgs a = args_of(tv, tv->n, tv->ns_h, tv->ns_f);
  a.rt_inl = tv->d_in_status;
  HS_TV_LAUNCH(hs_k_tv_begin, dim3(1), 256, -1);
  HS_TV_LAUNCH(hs_k_tv_check_rt, dim3(blocks(tv->n), kTvMaxRt), 256, -1);
  HS_TV_LAUNCH(hs_k_tv_select, dim3(kTvMaxRt), 256, -1);
  HS_HIP(hipStreamSynchronize(s));
  return HS_OK;
}

}  // extern "C"
