// hs_map_host.h — the point map (private to the library): the device store of retired points, the host-side run
// table and counters per keyframe, and what hs_ba_window.cpp calls when a window with an attached map loses points.
// Shared by hs_map.cpp (the ABI of include/hs_map.h) and hs_ba_window.cpp (the removals).
#pragma once
#include <unordered_map>
#include <utility>
#include <vector>

#include "hs_ba_ctx.h"
#include "hs_map_kernels.h"

namespace hs {
constexpr int kMapMaxRuns = 4096;  // record runs of one keyframe a cloud refresh can name (one per retire call at most)

// what the map knows about one keyframe without touching the device
struct MapFrame {
  int n_marg = 0, n_out = 0;                 // pointHessiansMarginalized.size(), pointHessiansOut.size()
  std::vector<std::pair<int, int>> runs;     // (first record, count): its records, both statuses, in push order
};
}  // namespace hs

struct hs_map : hs::Device {
  hs::Pool pool;
  int capacity = 0, n_rec = 0;
  hs_ctx* owner = nullptr;                   // the context it is attached to
  std::unordered_map<int, hs::MapFrame> frames;  // by hs_frame.id
  hs_map_record* d_rec = nullptr;            // [capacity]
  // a retire's inputs: the committed positions (ranked on the device into d_list, or written by the host), the handles
  // and statuses (written by the host into the mapped pinned block the kernel reads in place)
  int* d_list = nullptr;
  uint8_t* h_up = nullptr;                   // pinned: [capacity] positions | [capacity] handles | [capacity] statuses
  uint8_t* d_up = nullptr;                   // the device view of h_up
  hipEvent_t ev_up = nullptr;                // the last retire launch that reads h_up
  // the display cloud of the last refresh
  float* d_xyz = nullptr;                    // [capacity * 8][3]
  uint8_t* d_rgb = nullptr;                  // [capacity * 8][3]
  int *d_runs = nullptr, *h_runs = nullptr;  // [(kMapMaxRuns + 1) * 2] run table of a refresh (pinned staging)
  int *d_out = nullptr, *h_out = nullptr;    // [8] vertex count + the intrinsics' bits
  uint8_t* d_flags = nullptr;                // [HS_MAXF] hs_k_win_flag_frames' result
  int cloud_n = 0;

  int* up_list() const { return reinterpret_cast<int*>(h_up); }
  int* up_handle() const { return reinterpret_cast<int*>(h_up) + capacity; }
  uint8_t* up_status() const { return h_up + 8 * (size_t)capacity; }
};

namespace hs {
// hs_map.cpp.  The context's committed window is the source of every value: positions are committed positions, whose
// device state pending edits leave in place until the next commit.
// map_retire_flagged: the action != 0 points of h_action[nP] (n of them; d_flag_action holds the same bytes) become
// records; HS_ERR_NOMEM before anything has changed when they do not fit.
int map_retire_flagged(hs_ctx* c, const uint8_t* h_action, int n);
// map_retire_listed: n committed positions / handles / statuses, in push order.
int map_room(hs_ctx* c, int n);   // HS_ERR_NOMEM when n more records do not fit
int map_retire_listed(hs_ctx* c, int n, const int* pos, const int* handles, const uint8_t* status);
void map_forget(hs_ctx* c);       // the context goes away (or detaches): the map has no owner
}  // namespace hs
