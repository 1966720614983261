// hs_map.cpp — the point map of include/hs_map.h: what Frame::pointHessiansMarginalized / pointHessiansOut keep in
// the reference (Src/Mapping.cpp:272,300,306,313; Src/FullSystemOptimize.cpp:589), as an append-only store of 64-byte
// records on the device, KFDisplay::RefreshPC over it (Src/Display.cpp:382-513) and
// System::flagFramesForMarginalization (Src/FullSystemMarginalize.cpp:18-103), which counts it.
//
// The records are written by hs_k_map_retire on the attached context's stream, between the decision and the removal
// of the points (hs_ba_window.cpp calls map_rank_flagged / map_retire_flagged / map_retire_listed).  The host keeps,
// per keyframe id, the two counters and the runs of its records, derived from what the callers already know (the
// action bytes, the mirror): no record is read back to account for it.  While a map is attached everything of it is
// ordered on the context's stream; a detached map uses its own.
#include <algorithm>
#include <cstring>

#include "hs_map_host.h"

using namespace hs;

namespace {

hipStream_t map_stream(hs_map* m) { return m->owner ? m->owner->stream : m->stream; }

int map_wait(hs_map* m) {
  if (m->owner) return wait_stream(m->owner);
  HS_HIP(hipStreamSynchronize(m->stream));
  return HS_OK;
}

// one more record of keyframe `id`, the map's record `idx`
void account(hs_map* m, int id, int status, int idx) {
  MapFrame& f = m->frames[id];
  (status == HS_PT_MARGINALIZED ? f.n_marg : f.n_out)++;
  if (!f.runs.empty() && f.runs.back().first + f.runs.back().second == idx) f.runs.back().second++;
  else f.runs.push_back({idx, 1});
}

int frame_id_of(const hs_ctx* c, int f) { return c->h_state->frames[f].id; }

// The launch of hs_k_map_retire for n points on the context's stream.  Their handles are in m->up_handle(); their
// positions in m->d_list (ranked on the device) or, with list_from_host, in m->up_list(); their statuses come from
// d_action or from m->up_status().  The kernel reads the host-written lists through the mapped pinned block (a few
// bytes per point over the link, no copy to enqueue); ev_up marks when the host may write the block again.
int launch_retire(hs_ctx* c, int n, const uint8_t* d_action, bool list_from_host) {
  hs_map* m = c->map;
  hipStream_t s = c->stream;
  HsMapRetireArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n = n;
  a.list = list_from_host ? reinterpret_cast<const int*>(m->d_up) : m->d_list;
  a.handle = reinterpret_cast<const int*>(m->d_up) + m->capacity;
  a.action = d_action;
  a.status = m->d_up + 8 * (size_t)m->capacity;
  for (int f = 0; f < HS_MAXF; f++) a.frame_id[f] = f < c->nF ? frame_id_of(c, f) : 0;
  a.pt_host = c->d_pt_host;
  a.u = c->d_u;
  a.v = c->d_v;
  a.idepth = c->d_idepth;
  a.idepth_zero = c->d_idepth_zero;
  a.hdif = c->hdif_solved;
  a.relBL = c->d_fix_relBL;
  a.color = c->d_color;
  a.nGood = c->d_fix_nGood;
  a.rec = m->d_rec + m->n_rec;
  hipLaunchKernelGGL(hs_k_map_retire, dim3((n * 4 + 255) / 256), dim3(256), 0, s, a);
  HS_HIP(hipGetLastError());
  HS_HIP(hipEventRecord(m->ev_up, s));
  return HS_OK;
}

}  // namespace

namespace hs {

void map_forget(hs_ctx* c) {
  if (c->map) c->map->owner = nullptr;
  c->map = nullptr;
}

int map_room(hs_ctx* c, int n) {
  const hs_map* m = c->map;
  if (n > m->capacity - m->n_rec)
    return fail(HS_ERR_NOMEM, "the map's capacity is exhausted: " + std::to_string(m->n_rec) + " records + " +
                                  std::to_string(n) + " > " + std::to_string(m->capacity));
  return HS_OK;
}

int map_retire_flagged(hs_ctx* c, const uint8_t* h_action, int n) {
  hs_map* m = c->map;
  HS_TRY(map_room(c, n));
  if (n == 0) return HS_OK;
  HS_HIP(hipEventSynchronize(m->ev_up));  // the last retire has read the pinned block
  int* hh = m->up_handle();
  int q = 0;
  for (int p = 0; p < c->nP && q < n; p++)
    if (h_action[p]) hh[q++] = c->pt_handle[p];
  if (q != n) return fail(HS_ERR_STATE, "the action bytes and their counters disagree");
  // the leaving points' positions in window order: a stable compaction of the actions the decision kernel left on the
  // device (nothing of it is read back; it runs behind the call's read-back, not in front of it)
  hipLaunchKernelGGL(hs_k_map_rank, dim3(1), dim3(1024), 0, c->stream, c->nP, c->d_flag_action, m->d_list,
                     m->capacity, (int*)nullptr);
  HS_HIP(hipGetLastError());
  HS_TRY(launch_retire(c, n, c->d_flag_action, false));
  q = 0;
  for (int p = 0; p < c->nP; p++)
    if (h_action[p])
      account(m, frame_id_of(c, c->pt_host[p]), h_action[p] == 2 ? HS_PT_MARGINALIZED : HS_PT_OUTLIER, m->n_rec + q++);
  m->n_rec += n;
  return HS_OK;
}

int map_retire_listed(hs_ctx* c, int n, const int* pos, const int* handles, const uint8_t* status) {
  hs_map* m = c->map;
  HS_TRY(map_room(c, n));
  if (n == 0) return HS_OK;
  HS_HIP(hipEventSynchronize(m->ev_up));
  std::memcpy(m->up_list(), pos, sizeof(int) * (size_t)n);
  std::memcpy(m->up_handle(), handles, sizeof(int) * (size_t)n);
  std::memcpy(m->up_status(), status, (size_t)n);
  HS_TRY(launch_retire(c, n, nullptr, true));
  for (int i = 0; i < n; i++) account(m, frame_id_of(c, c->pt_host[pos[i]]), status[i], m->n_rec + i);
  m->n_rec += n;
  return HS_OK;
}

}  // namespace hs

extern "C" {

int hs_map_create(hs_map** out, int capacity_points, int device_id) {
  if (!out) return fail(HS_ERR_INVALID, "null out");
  *out = nullptr;
  if (capacity_points <= 0 || capacity_points > (1 << 26)) return fail(HS_ERR_INVALID, "bad map capacity");
  HS_TRY(check_device(device_id));
  hs_map* m = new hs_map();
  m->capacity = capacity_points;
  const size_t cap = (size_t)capacity_points;
  const int rc = [&]() -> int {
    HS_TRY(m->open(device_id));
    HS_TRY(m->pool.alloc_zero(&m->d_rec, cap, m->stream));
    HS_TRY(m->pool.alloc(&m->d_list, cap));
    HS_TRY(m->pool.pinned(&m->h_up, 9 * cap, hipHostMallocMapped));
    HS_HIP(hipHostGetDevicePointer((void**)&m->d_up, m->h_up, 0));
    HS_TRY(m->pool.alloc(&m->d_xyz, cap * 24));
    HS_TRY(m->pool.alloc(&m->d_rgb, cap * 24));
    HS_TRY(m->pool.alloc(&m->d_runs, (size_t)(kMapMaxRuns + 1) * 2));
    HS_TRY(m->pool.pinned(&m->h_runs, (size_t)(kMapMaxRuns + 1) * 2));
    HS_TRY(m->pool.alloc_zero(&m->d_out, 8, m->stream));
    HS_TRY(m->pool.pinned(&m->h_out, 8));
    HS_TRY(m->pool.alloc_zero(&m->d_flags, HS_MAXF, m->stream));
    HS_HIP(hipEventCreateWithFlags(&m->ev_up, hipEventDisableTiming));
    HS_HIP(hipEventRecord(m->ev_up, m->stream));
    HS_HIP(hipStreamSynchronize(m->stream));
    return HS_OK;
  }();
  if (rc) hs_map_destroy(m);
  else *out = m;
  return rc;
}

void hs_map_destroy(hs_map* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  if (m->owner) {  // still attached: the owner's queued retires finish, then it forgets the map
    if (m->owner->stream) (void)hipStreamSynchronize(m->owner->stream);
    map_forget(m->owner);
  }
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  m->pool.release_all();
  if (m->ev_up) (void)hipEventDestroy(m->ev_up);
  m->close();
  delete m;
}

int hs_ba_attach_map(hs_ctx* c, hs_map* m) {
  if (!c) return fail(HS_ERR_INVALID, "null context");
  if (c->comm_lost) return fail(HS_ERR_RCCL, "communicator aborted by an earlier call (a peer rank failed)");
  if (!m) {  // detach: the retires already queued finish first, so the map can go on alone
    if (c->map) {
      HS_HIP(hipSetDevice(c->device));
      HS_TRY(wait_stream(c));
      map_forget(c);
    }
    return HS_OK;
  }
  if (c->multi_rank()) return fail(HS_ERR_STATE, "hs_ba_attach_map needs a single-rank context");
  if (m->device != c->device) return fail(HS_ERR_INVALID, "the map is on another device than the context");
  if (m->owner && m->owner != c) return fail(HS_ERR_STATE, "the map is attached to another context");
  if (c->map && c->map != m) return fail(HS_ERR_STATE, "the context has a map attached (detach it first)");
  HS_HIP(hipSetDevice(c->device));
  HS_HIP(hipStreamSynchronize(m->stream));  // the map's own work so far precedes the context's stream
  c->map = m;
  m->owner = c;
  return HS_OK;
}

int hs_map_retire_points(hs_ctx* c, int n, const int* handles, const uint8_t* status) {
  if (!c) return fail(HS_ERR_INVALID, "null context");
  if (!c->map) return fail(HS_ERR_STATE, "no map attached (hs_ba_attach_map)");
  if (n < 0 || (n > 0 && (!handles || !status))) return fail(HS_ERR_INVALID, "bad point list");
  HS_TRY(hs_ba_make_idx(c, nullptr, nullptr, nullptr));
  std::vector<int> pos(n);
  std::vector<uint8_t> seen(c->nP, 0);
  for (int i = 0; i < n; i++) {
    if (status[i] != HS_PT_OUTLIER && status[i] != HS_PT_MARGINALIZED)
      return fail(HS_ERR_INVALID, "a retired point's status must be HS_PT_OUTLIER or HS_PT_MARGINALIZED");
    const int h = handles[i];
    int p = -1;
    if (h >= 0 && h < (int)c->loc_key.size() && c->loc_key[h] >= 0)
      for (int f = 0; f < (int)c->wframes.size(); f++)
        if (c->wframes[f].key == c->loc_key[h]) p = c->wpts[f][c->loc_idx[h]].src;
    if (p < 0 || p >= c->nP || c->pt_handle[p] != h || seen[p])
      return fail(HS_ERR_INVALID, "a handle is not in the committed window (or is listed twice)");
    seen[p] = 1;
    pos[i] = p;
  }
  return map_retire_listed(c, n, pos.data(), handles, status);
}

int hs_map_size(hs_map* m, int* n_records, int* n_frames) {
  if (!m) return fail(HS_ERR_INVALID, "null map");
  if (n_records) *n_records = m->n_rec;
  if (n_frames) *n_frames = (int)m->frames.size();
  return HS_OK;
}

int hs_map_frame_counts(hs_map* m, int frame_id, int* n_marginalized, int* n_out) {
  if (!m) return fail(HS_ERR_INVALID, "null map");
  const auto it = m->frames.find(frame_id);
  if (n_marginalized) *n_marginalized = it == m->frames.end() ? 0 : it->second.n_marg;
  if (n_out) *n_out = it == m->frames.end() ? 0 : it->second.n_out;
  return HS_OK;
}

int hs_map_get_records(hs_map* m, int first, int n, hs_map_record* out) {
  if (!m) return fail(HS_ERR_INVALID, "null map");
  if (first < 0 || n < 0 || first > m->n_rec || n > m->n_rec - first || (n > 0 && !out))
    return fail(HS_ERR_INVALID, "record range outside the map");
  if (n == 0) return HS_OK;
  HS_HIP(hipSetDevice(m->device));
  HS_HIP(hipMemcpyAsync(out, m->d_rec + first, sizeof(hs_map_record) * (size_t)n, hipMemcpyDeviceToHost, map_stream(m)));
  return map_wait(m);
}

int hs_map_clear(hs_map* m) {
  if (!m) return fail(HS_ERR_INVALID, "null map");
  m->n_rec = 0;
  m->frames.clear();
  m->cloud_n = 0;
  return HS_OK;
}

int hs_map_refresh_cloud(hs_map* m, hs_ctx* c, int frame_id, float* xyz_out, uint8_t* rgb_out, int cap, int* n_out,
                         float* kinv_out) {
  if (!m) return fail(HS_ERR_INVALID, "null map");
  if (cap < 0) return fail(HS_ERR_INVALID, "bad cloud capacity");
  if (!c) return fail(HS_ERR_INVALID, "null context (the cloud's intrinsics are the window's calibration)");
  if (m->owner && m->owner != c) return fail(HS_ERR_STATE, "the map is attached to another context");
  if (c->device != m->device) return fail(HS_ERR_INVALID, "the map is on another device than the context");
  HS_HIP(hipSetDevice(m->device));
  HsMapCloudArgs a;
  std::memset(&a, 0, sizeof(a));
  HS_TRY(hs_ba_make_idx(c, nullptr, nullptr, nullptr));
  for (int f = 0; f < c->nF; f++)
    if (c->h_state->frames[f].id == frame_id) {
      a.act_begin = c->host_pt_begin[f];
      a.act_n = c->host_pt_begin[f + 1] - c->host_pt_begin[f];
      break;
    }
  a.u = c->d_u;
  a.v = c->d_v;
  a.idepth = c->d_idepth;
  a.hdif = c->hdif_solved;
  a.relBL = c->d_fix_relBL;
  a.st = c->d_state;
  hipStream_t s = c->stream;
  // the frame's runs with the number of candidates before each; the closing entry holds their total
  const auto it = m->frames.find(frame_id);
  int n_runs = 0, total = 0;
  if (it != m->frames.end() && it->second.n_marg > 0) {
    const auto& runs = it->second.runs;
    if ((int)runs.size() > kMapMaxRuns) return fail(HS_ERR_NOMEM, "the keyframe's records lie in too many runs");
    for (const auto& r : runs) {
      m->h_runs[2 * n_runs] = r.first;
      m->h_runs[2 * n_runs + 1] = total;
      total += r.second;
      n_runs++;
    }
    m->h_runs[2 * n_runs] = 0;
    m->h_runs[2 * n_runs + 1] = total;
    HS_HIP(hipMemcpyAsync(m->d_runs, m->h_runs, sizeof(int) * 2 * (size_t)(n_runs + 1), hipMemcpyHostToDevice, s));
  }
  if (a.act_n + total > m->capacity) return fail(HS_ERR_NOMEM, "the keyframe's cloud exceeds the map's capacity");
  a.n_runs = n_runs;
  a.runs = m->d_runs;
  a.rec = m->d_rec;
  a.xyz = m->d_xyz;
  a.rgb = m->d_rgb;
  a.cap_pts = m->capacity;
  a.out = m->d_out;
  hipLaunchKernelGGL(hs_k_map_cloud, dim3(1), dim3(HS_MAP_CLOUD_NT), 0, s, a);
  HS_HIP(hipGetLastError());
  HS_HIP(hipMemcpyAsync(m->h_out, m->d_out, sizeof(int) * 8, hipMemcpyDeviceToHost, s));
  HS_TRY(wait_stream(c));
  const int n = m->h_out[0];
  m->cloud_n = n;
  if (n_out) *n_out = n;
  if (kinv_out) std::memcpy(kinv_out, m->h_out + 1, 4 * sizeof(float));
  const size_t take = (size_t)std::min(n, cap);
  if (take > 0 && (xyz_out || rgb_out)) {
    if (xyz_out) HS_HIP(hipMemcpyAsync(xyz_out, m->d_xyz, take * 12, hipMemcpyDeviceToHost, s));
    if (rgb_out) HS_HIP(hipMemcpyAsync(rgb_out, m->d_rgb, take * 3, hipMemcpyDeviceToHost, s));
    HS_TRY(wait_stream(c));
  }
  return HS_OK;
}

int hs_map_cloud_device(hs_map* m, const float** d_xyz, const uint8_t** d_rgb, int* n) {
  if (!m) return fail(HS_ERR_INVALID, "null map");
  if (d_xyz) *d_xyz = m->d_xyz;
  if (d_rgb) *d_rgb = m->d_rgb;
  if (n) *n = m->cloud_n;
  return HS_OK;
}

int hs_frame_marg_params_default(hs_frame_marg_params* p) {
  if (!p) return fail(HS_ERR_INVALID, "null params");
  p->minFrameAge = 1;
  p->maxFrames = 7;
  p->minFrames = 5;
  p->minPointsRemaining = 0.05f;
  p->maxLogAffFacInWindow = 0.7f;
  return HS_OK;
}

int hs_ba_flag_frames_for_marginalization(hs_ctx* c, const hs_frame_marg_params* params, const int* kf_id,
                                          const int* n_immature, uint8_t* flagged_out, int* n_flagged) {
  if (!c) return fail(HS_ERR_INVALID, "null context");
  if (c->comm_lost) return fail(HS_ERR_RCCL, "communicator aborted by an earlier call (a peer rank failed)");
  if (!c->map) return fail(HS_ERR_STATE, "hs_ba_flag_frames_for_marginalization needs an attached map");
  if (!kf_id) return fail(HS_ERR_INVALID, "null kf_id");
  HS_TRY(hs_ba_make_idx(c, nullptr, nullptr, nullptr));
  if (c->nF == 0) return fail(HS_ERR_STATE, "no window");
  hs_map* m = c->map;
  HsFlagFramesArgs a;
  std::memset(&a, 0, sizeof(a));
  a.nF = c->nF;
  a.st = c->d_state;
  if (params) a.P = *params;
  else hs_frame_marg_params_default(&a.P);
  for (int f = 0; f < c->nF; f++) {
    a.in[f] = c->host_pt_begin[f + 1] - c->host_pt_begin[f] + (n_immature ? n_immature[f] : 0);
    int nm = 0, no = 0;
    hs_map_frame_counts(m, frame_id_of(c, f), &nm, &no);
    a.out[f] = nm + no;
    a.kf_id[f] = kf_id[f];
  }
  a.flagged = m->d_flags;
  hipLaunchKernelGGL(hs_k_win_flag_frames, dim3(1), dim3(64), 0, c->stream, a);
  HS_HIP(hipGetLastError());
  const uint8_t* h_flags = reinterpret_cast<const uint8_t*>(m->h_out);  // the map's pinned word block
  HS_HIP(hipMemcpyAsync(m->h_out, m->d_flags, HS_MAXF, hipMemcpyDeviceToHost, c->stream));
  HS_TRY(wait_stream(c));
  int n = 0;
  for (int f = 0; f < c->nF; f++) {
    if (flagged_out) flagged_out[f] = h_flags[f];
    n += h_flags[f] != 0;
  }
  if (n_flagged) *n_flagged = n;
  return HS_OK;
}

}  // extern "C"

// the CPU test's entry to hs::frame_rule (tests/test_frame_rule.py): no device work
extern "C" int hs_debug_frame_rule(int nF, const int* in, const int* out, const double* aff0, const float* dist,
                                   const int* kf_id, const hs_frame_marg_params* P, uint8_t* flagged, uint8_t* why) {
  if (nF < 0 || nF > HS_MAXF || !P) return -1;
  return hs::frame_rule(nF, in, out, aff0, dist, kf_id, *P, flagged, why);
}
