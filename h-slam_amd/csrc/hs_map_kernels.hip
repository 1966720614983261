// hs_map_kernels.hip — device side of the point map (hs_map.cpp, include/hs_map.h).
//
//   hs_k_map_rank         stable compaction of hs_k_win_flag's actions: the committed positions of the points that
//                         leave, in window order (the reference's push order).  One workgroup, ballot prefix sums per
//                         chunk, as hs_k_win_newest.
//   hs_k_map_retire       one 64-byte record per point that leaves, from the window's device-resident state.  One lane
//                         per (point, 16-byte quarter of the record): a wave stores 1 KiB of consecutive bytes.
//   hs_k_map_cloud        KFDisplay::RefreshPC (Src/Display.cpp:382-513) for one keyframe: its active points, then its
//                         marginalized records, filtered and expanded to 8 vertices + colours each, compacted in order.
//                         One workgroup, one lane per (point, pattern pixel): the filter is uniform over a point's 8
//                         lanes, a chunk's kept points are ranked by ballots, and the lanes store consecutive vertices.
//   hs_k_win_flag_frames  System::flagFramesForMarginalization (hs_frame_rule.h): one wave forms the affine factors and
//                         the pair distances from the device-resident frame state, lane 0 applies the rule.
#include <hip/hip_runtime.h>

#include "hs_imm_ctor.h"
#include "hs_map_kernels.h"

__global__ __launch_bounds__(1024) void hs_k_map_rank(int n, const uint8_t* __restrict__ action,
                                                      int* __restrict__ list, int cap, int* __restrict__ n_out) {
  __shared__ int wsum[16];
  __shared__ int base_s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int c0 = 0; c0 < n; c0 += 1024) {
    const int p = c0 + tid;
    const bool take = p < n && action[p] != 0;
    const unsigned long long m = __ballot(take);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    int off = base_s;
    for (int w = 0; w < wv; w++) off += wsum[w];
    if (take && off + before < cap) list[off + before] = p;
    __syncthreads();
    if (tid == 0) {
      int s = 0;
      for (int w = 0; w < 16; w++) s += wsum[w];
      base_s += s;
    }
    __syncthreads();
  }
  if (tid == 0 && n_out) *n_out = base_s;
}

// window frame -> hs_frame.id: a select chain over the uniform kernel arguments (no per-lane table load)
__device__ __forceinline__ int map_frame_id(const int (&id)[HS_MAXF], int h) {
  int r = id[0];
#pragma unroll
  for (int i = 1; i < HS_MAXF; i++) r = (h == i) ? id[i] : r;
  return r;
}

// Vec3b(color, color, color): float -> unsigned char, truncation toward zero
__device__ __forceinline__ unsigned map_color_u8(float c) { return (unsigned)(int)c & 0xffu; }

__global__ __launch_bounds__(256) void hs_k_map_retire(HsMapRetireArgs a) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = gid >> 2, q = gid & 3;
  if (i >= a.n) return;
  const int p = a.list[i];
  uint4 w = make_uint4(0u, 0u, 0u, 0u);
  if (q == 0) {
    const int st = a.action ? (a.action[p] == 2 ? HS_PT_MARGINALIZED : HS_PT_OUTLIER) : (int)a.status[i];
    w = make_uint4((unsigned)a.handle[i], (unsigned)map_frame_id(a.frame_id, a.pt_host[p]), (unsigned)st,
                   (unsigned)a.nGood[p]);
  } else if (q == 1) {
    w = make_uint4(__float_as_uint(a.u[p]), __float_as_uint(a.v[p]), __float_as_uint(a.idepth[p]),
                   __float_as_uint(a.idepth_zero[p]));
  } else if (q == 2) {
    const float4 c0 = reinterpret_cast<const float4*>(a.color)[(size_t)p * 2];
    const float4 c1 = reinterpret_cast<const float4*>(a.color)[(size_t)p * 2 + 1];
    const unsigned lo = map_color_u8(c0.x) | (map_color_u8(c0.y) << 8) | (map_color_u8(c0.z) << 16) |
                        (map_color_u8(c0.w) << 24);
    const unsigned hi = map_color_u8(c1.x) | (map_color_u8(c1.y) << 8) | (map_color_u8(c1.z) << 16) |
                        (map_color_u8(c1.w) << 24);
    w = make_uint4(__float_as_uint(a.hdif[p]), __float_as_uint(a.relBL[p]), lo, hi);
  }
  reinterpret_cast<uint4*>(a.rec)[(size_t)i * 4 + q] = w;
}

__global__ __launch_bounds__(HS_MAP_CLOUD_NT) void hs_k_map_cloud(HsMapCloudArgs a) {
  __shared__ int wsum[HS_MAP_CLOUD_NT / 64];
  __shared__ int base_s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int pt = tid >> 3, k = tid & 7;
  const float fxi = a.st->calib.value_scaledi[0], fyi = a.st->calib.value_scaledi[1];
  const float cxi = a.st->calib.value_scaledi[2], cyi = a.st->calib.value_scaledi[3];
  if (tid == 0) base_s = 0;
  __syncthreads();
  const int n_rec = a.n_runs > 0 ? a.runs[2 * a.n_runs + 1] : 0;
  const int total = a.act_n + n_rec;
  for (int c0 = 0; c0 < total; c0 += HS_MAP_CLOUD_PTS) {
    const int j = c0 + pt;
    bool have = false, active = false;
    float u = 0.f, v = 0.f, idepth = 0.f, hdif = 0.f, relBL = 0.f;
    unsigned col = 0;
    if (j < a.act_n) {
      const int p = a.act_begin + j;
      have = active = true;
      u = a.u[p]; v = a.v[p]; idepth = a.idepth[p]; hdif = a.hdif[p]; relBL = a.relBL[p];
    } else if (j < total) {
      const int jr = j - a.act_n;
      int r = 0;
      while (r + 1 < a.n_runs && jr >= a.runs[2 * (r + 1) + 1]) r++;
      const hs_map_record& R = a.rec[a.runs[2 * r] + (jr - a.runs[2 * r + 1])];
      if (R.status == HS_PT_MARGINALIZED) {
        have = true;
        u = R.u; v = R.v; idepth = R.idepth; hdif = R.hdif; relBL = R.maxRelBaseline;
        col = R.color[k];
      }
    }
    bool keep = have && !(idepth < 0);
    float depth = 0.f;
    if (keep) {
      depth = __fdiv_rn(1.0f, idepth);
      float depth4 = __fmul_rn(depth, depth);
      depth4 = __fmul_rn(depth4, depth4);
      const float ih = hdif > 0 ? (float)(1.0 / (double)hdif) : 0.f;
      const float var = (float)(1.0 / ((double)ih + 0.01));
      if (__fmul_rn(var, depth4) > 0.001f) keep = false;
      if (var > 0.001f) keep = false;
      if (relBL < 0.1f) keep = false;
    }
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << (lane & ~7)) - 1ull)) >> 3;  // kept points below this lane's point
    if (lane == 0) wsum[wv] = __popcll(m) >> 3;
    __syncthreads();
    int off = base_s;
    for (int w = 0; w < wv; w++) off += wsum[w];
    off += before;
    if (keep && off < a.cap_pts) {
      const size_t o = ((size_t)off * 8 + k) * 3;
      // ((u + dx) * fxi + cxi) * depth, every operation rounded on its own
      a.xyz[o] = __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(u, (float)hs_imm::kPat[k][0]), fxi), cxi), depth);
      a.xyz[o + 1] = __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(v, (float)hs_imm::kPat[k][1]), fyi), cyi), depth);
      a.xyz[o + 2] = depth;
      a.rgb[o] = active ? (uint8_t)0 : (uint8_t)col;
      a.rgb[o + 1] = active ? (uint8_t)0 : (uint8_t)col;
      a.rgb[o + 2] = active ? (uint8_t)255 : (uint8_t)col;
    }
    __syncthreads();
    if (tid == 0) {
      int s = 0;
      for (int w = 0; w < HS_MAP_CLOUD_NT / 64; w++) s += wsum[w];
      base_s += s;
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.out[0] = base_s * 8;
    a.out[1] = (int)__float_as_uint(fxi);
    a.out[2] = (int)__float_as_uint(fyi);
    a.out[3] = (int)__float_as_uint(cxi);
    a.out[4] = (int)__float_as_uint(cyi);
  }
}

__global__ __launch_bounds__(64) void hs_k_win_flag_frames(HsFlagFramesArgs a) {
  __shared__ float dist[HS_MAXF * HS_MAXF];
  __shared__ double aff0[HS_MAXF];
  __shared__ int in_s[HS_MAXF], out_s[HS_MAXF], kf_s[HS_MAXF];
  __shared__ uint8_t flag_s[HS_MAXF];
  const int lane = threadIdx.x;
  const int nF = a.nF;
  if (lane < HS_MAXF) {
    int vi = a.in[0], vo = a.out[0], vk = a.kf_id[0];
#pragma unroll
    for (int i = 1; i < HS_MAXF; i++) {
      vi = lane == i ? a.in[i] : vi;
      vo = lane == i ? a.out[i] : vo;
      vk = lane == i ? a.kf_id[i] : vk;
    }
    in_s[lane] = vi;
    out_s[lane] = vo;
    kf_s[lane] = vk;
    flag_s[lane] = 0;
  }
  // FrameFramePrecalc::distanceLL of (host h, target t): |(T.PRE_worldToCam * H.PRE_camToWorld).translation()|, a float
  {
    const int h = lane / nF, t = lane % nF;
    if (h < nF) {
      const hs::FrameH& H = a.st->frames[h];
      const hs::FrameH& T = a.st->frames[t];
      double rt[3];
      hs::qrot(T.PRE_worldToCam.q, H.PRE_camToWorld.t, rt);
      const double x = T.PRE_worldToCam.t[0] + rt[0], y = T.PRE_worldToCam.t[1] + rt[1],
                   z = T.PRE_worldToCam.t[2] + rt[2];
      dist[h * nF + t] = (float)sqrt(x * x + y * y + z * z);
    }
  }
  // refToFh[0] of AffLight::fromToVecExposure(newest, frame)
  if (lane < nF) {
    const hs::FrameH& N = a.st->frames[nF - 1];
    const hs::FrameH& F = a.st->frames[lane];
    double ab[2];
    hs::fromToVecExposure(N.ab_exposure, F.ab_exposure, N.aff_a(), N.aff_b(), F.aff_a(), F.aff_b(), ab);
    aff0[lane] = ab[0];
  }
  __syncthreads();
  if (lane == 0) hs::frame_rule(nF, in_s, out_s, aff0, dist, kf_s, a.P, flag_s, nullptr);
  __syncthreads();
  if (lane < HS_MAXF) a.flagged[lane] = flag_s[lane];
}
