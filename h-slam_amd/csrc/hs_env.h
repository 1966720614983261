// hs_env.h — every environment switch of the library, and the only file that calls getenv.  A switch is kept while a
// test, bench.py or a tool sets it; an A/B path that was measured and lost is a patch on a branch (Makefile: variant),
// not a switch.  Each block below says what the switch selects, where it is read -- at context creation, at the window
// commit (make_partition: every hs_ba_set_window and incremental commit) or per call -- and who sets it.
// INTEGRATION.md ("Diagnostics") carries the same list for callers.
#pragma once
#include <cstdlib>

namespace hs {
namespace env {

// "1" is on, any other value off; unset: dflt
inline bool flag(const char* name, bool dflt) {
  const char* e = std::getenv(name);
  return e ? e[0] == '1' : dflt;
}
inline int num(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : dflt;
}

// ---------------------------------------------------------------- BA path selection (hs_ba.cpp)
// HS_ACC_EXACT=1: one linearize block per host whose wave 0 takes every point in order (the single-thread reference's
// fp32 accumulator sums; at most 1000 points per host).  Window commit.  tests/test_gpu_ba.py, tests/test_golden.py.
inline bool acc_exact() { return flag("HS_ACC_EXACT", false); }
// HS_LIN8=0 / 1: hs_k_lin / hs_k_lin8 whatever the window's size (unset: hs_k_lin8 from kLin8MinPoints points).
// Window commit.  tests/test_gpu_lin8.py, tests/test_gpu_fp64_model.py.
inline bool lin8(bool dflt) { return flag("HS_LIN8", dflt); }
// HS_LIN8_NOFILL=1: hs_k_lin8's plain ceil partition, without the blocks that fill the grid.  Window commit.
// tests/test_gpu_lin8.py.
inline bool lin8_nofill() { return flag("HS_LIN8_NOFILL", false); }
// HS_LIN8_HIST=0: setNewFrameEnergyTH's pass-1 histogram by hs_k_reduce's blocks instead of inside hs_k_lin8.
// Window commit.  tests/test_gpu_lin8.py.
inline bool lin8_hist() { return flag("HS_LIN8_HIST", true); }
// HS_TH_MULTI=0 / 1: the threshold select as one block / as the multi-block passes 2 and 3 (unset: multi-block from
// kThMultiMinPoints points).  Window commit.  tests/test_gpu_lin8.py, tests/test_gpu_ba.py, tests/test_gpu_shard.py.
inline bool th_multi(bool dflt) { return flag("HS_TH_MULTI", dflt); }
// HS_GRAPH=1: the GN loop replays iteration pairs as one captured hipGraph.  Window commit.  tests/test_gpu_ba.py.
inline bool graph() { return flag("HS_GRAPH", false); }
// HS_HOST_BREAK=1: the GN loop reads canbreak back after every iteration instead of breaking on the device.
// Window commit.  tests/test_gpu_ba.py.
inline bool host_break() { return flag("HS_HOST_BREAK", false); }
// HS_EVENT_TIMING=n: HIP event pairs inside the GN loop, the default of hs_ba_set_event_timing (1: around the
// linearize kernel, 2: around every phase).  Context creation.  bench.py (--phase-events), tests/test_gpu_bench.py.
inline int event_timing() { return num("HS_EVENT_TIMING", 0); }

// ---------------------------------------------------------------- tracker (hs_track.cpp: one block in run_tries)
// HS_TRK_G=n: at most n workgroups per hypothesis, within the co-residency cap (1: the one-workgroup LM loop).
// Per call.  tests/test_gpu_track.py.
inline int trk_g(int dflt) { return num("HS_TRK_G", dflt); }
// HS_TRK_G_UNCHECKED=n: n workgroups per hypothesis past the co-residency cap, so that meetings time out (test hook).
// Per call.  tests/test_gpu_track.py.
inline int trk_g_unchecked(int dflt) { return num("HS_TRK_G_UNCHECKED", dflt); }
// HS_TRK_SPIN=n: a member meeting's time bound in wall-clock ticks (unset or 0: 20 ms; test hook).  Per call.
// tests/test_gpu_track.py.
inline int trk_spin() { return num("HS_TRK_SPIN", 0); }
// HS_TRK_NOEVT=0 / 1: the event pair around the track launch on / off (unset: hs_tracker_set_event_timing decides;
// off, the host takes the results from the done words).  Per call.  tests/test_gpu_track.py.
inline bool trk_noevt(bool dflt) { return flag("HS_TRK_NOEVT", dflt); }

// ---------------------------------------------------------------- tracing
// HS_KTRACE=1: the kernels' clock stamps, summarised on stderr: the GN loop's kernels (BA context: where its buffers
// are allocated), hs_k_track (per call), hs_k_act_select's profile (tracer creation) and the refiner's step kernel
// (refiner creation).  tools/kexp.sh, tools/gpu_check.sh and the other trace runs under tools/.
inline bool ktrace() { return flag("HS_KTRACE", false); }

}  // namespace env
}  // namespace hs
