/*
 * hs_twoview.h — the initializer's two-view model fit on MI355X: Initializer::FindTransformation
 * (Src/Initializer.cpp:401-455) with FindHomography / FindFundamental (:457-555), ComputeH21 / ComputeF21 (:557-633),
 * CheckHomography / CheckFundamental (:635-809), ReconstructF / ReconstructH (:811-1073), Triangulate, Normalize,
 * CheckRT, DecomposeE (:1075-1281) and the median-depth scaling of Initialize (:142-148).
 *
 * Same conventions as hs_flow.h and hs_init.h: plain C, status codes from hs_types.h with the message in
 * hs_last_error(), the context owns its device memory and its own HIP stream, host buffers are the caller's and copied
 * in / out, every entry checks device, size and state before any device call, a failed entry changes nothing, and a
 * call is complete on the device when it returns.  Everything is allocated by hs_twoview_create; no later call
 * allocates.
 *
 * Not built: MatchIndirect, the stereo / RGBD initializers.  ColorVec is not kept: only its draws are consumed
 * (hs_twoview_rng_skip).
 *
 * Parity.  OpenCV is not a dependency of this project, so parity with cv::SVD is not pinned.  The contract below is
 * restated in numpy by tests/twoview_ref.py, which is what the kernels are held to.  Every deviation from the
 * reference is named.  All fp32 arithmetic is unfused, in the reference's operation order.
 *
 *   Keys.  xy1 = FirstFramePts, xy2 = MatchedPts, status = MatchedStatus, n of each.
 *   Fixed-order sum.  sum256(x_i) is the fp64 sum used wherever "summed in fp64" is said: partial[t] = the sum of
 *           x_i over i = t, t + 256, ... in ascending order, t = 0 .. 255; then for s = 128, 64, .. 1:
 *           partial[t] += partial[t + s] for t < s; the result is partial[0].
 *   Normalize (:1090-1136), for each image over all n keys (status 0 included, as the reference does):
 *           meanX = (float)(sum256(x) / n); devX = (float)(sum256(|x - meanX|) / n), the difference and fabs in fp32;
 *           sX = (float)(1.0 / devX); the normalized point is (x - meanX) * sX in fp32; T = [sX 0 -meanX*sX; 0 sY
 *           -meanY*sY; 0 0 1] in fp32.  The same for y.  Deviation: the reference sums sequentially in fp32.
 *   Hypotheses (:557-633), per set of 8 keys.  A (16 x 9 for H, 8 x 9 for F) is built from the fp32 normalized points
 *           in fp32 exactly as written, then widened.  In fp64: the null vector (the right singular vector of the
 *           smallest singular value, by the one-sided cyclic Jacobi of csrc/hs_jacobi.h: fixed sweep order, fixed
 *           stopping rule); for F the rank-2 projection (a second Jacobi on the 3 x 3 Fpre: Fn = the sum over the two
 *           larger columns j of (Fpre V)_j v_j^T); H21 = (T2^-1 Hn) T1 with T2^-1 = [1/sX 0 -c/sX; ...] from T2's fp32
 *           entries, H12 = adj(H21) / det(H21); F21 = (T2^T Fn) T1.  H21, H12 and F21 are rounded to fp32 once.
 *           Deviation: the reference rounds every intermediate to fp32 (cv::Mat products, cv::SVD).  The sign of a
 *           null vector is not part of the contract: every consumer is invariant to it.
 *   Scores (:635-809).  Per match with status != 0, in fp32 in the reference's order: th = 5.991 for H; th = 3.841
 *           with score constant 5.991 for F; sigma = 1.  The two contributions of match i are x_{2i}, x_{2i+1} (0
 *           where the reference adds nothing); score = (float)sum256 over matches of (x_{2i} + x_{2i+1} added in that
 *           order into the partial).  Deviation: the reference sums sequentially in fp32.  The winner is the lowest
 *           set that attains the maximum (the reference's strict >).  SH == 0 and SF == 0: why = 1.
 *   Model choice.  SH / (SH + SF) > 0.40 in fp32: H; else F.
 *   Motion hypotheses (:811-1073, :1261-1281).  In fp64 from the fp32 winner and the fp32 K: E = K^T F K or
 *           A = K^-1 H K, the 3 x 3 SVD by the same Jacobi (jacobi_svd3: U's third column is the cross product of the
 *           first two, which is what a rank-2 E leaves defined), the reference's formulas, d1/d2 and d2/d3 tested on
 *           the fp32-rounded singular values (why = 2).  The 4 (F: (R1,t) (R2,t) (R1,-t) (R2,-t)) or 8 (R, t) are
 *           rounded to fp32.
 *   CheckRT (:1138-1259), per inlier match and hypothesis.  P1 = K[I|0], P2 = K[R|t] and the rows of the 4 x 4 A in
 *           fp32; its null vector in fp64 (the same Jacobi); x3D = v[0..2] / v[3] in fp64, rounded to fp32; then
 *           every test in fp32 in the reference's order, with cv::norm and Mat::dot as fp64 sums of fp32 values:
 *           dist = (float)sqrt(sum x*x), cosParallax = (float)(dot / (double)(dist1 * dist2)).  Both of the
 *           reference's asymmetries are kept: nGood counts every match that passes, vbGood is set only where
 *           cosParallax < 0.99998.  The parallax is the order statistic at index min(50, size - 1) of the passing
 *           matches' cosParallax, selected exactly (radix select on the ordered bit pattern), then
 *           (float)((double)((float)acos((double)c) * 180.f) / pi); 0 when nothing passes.
 *   Decision.  csrc/hs_twoview_rule.h: ReconstructF's and ReconstructH's rules with minParallax = 1, minTriangulated =
 *           50; why = 3 or 4.
 *   Generator (randomGen, cv::RNG(0)).  Parity with OpenCV is not pinned; tests/initializer_ref.py restates this contract.
 *           State: one uint64_t.  seed(s): state = s ? s : 0xffffffff; create seeds with 0.
 *           next(): state = (uint64_t)(uint32_t)state * 4164903690u + (uint32_t)(state >> 32); returns (uint32_t)state.
 *           uniform(a, b): a == b ? a : (int)(next() % (unsigned)(b - a) + a); b is exclusive, a == b consumes no draw.
 *           From seed 0 the first four next() are 0x07c09cf6, 0xb302a6a5, 0xe6abd4e7, 0x507b8a5d and the state is then
 *           0xdfaf93c7507b8a5d (computed from this definition, a guard against 32- / 64-bit slips).
 *   Draw of mvSets (:404-432).  all = the indices i with status[i] != 0, ascending; m = |all|.  For every set it =
 *           0 .. n_sets-1: avail = all; for j = 0 .. 7: size = m - j; r = uniform(0, size - 1); sets[it][j] = avail[r];
 *           avail[r] = avail[size - 1]; pop.  The generator runs on through all sets and across calls.  With m == 8
 *           the eighth draw of every set is uniform(0, 0) and consumes nothing: 7 next() per set instead of 8.  m < 8
 *           is undefined behaviour in the reference; here it is refused and the state does not move.  The host runs
 *           the chain (8 * n_sets dependent multiply-adds at most) and uploads the 32-bit words; the list `all` and
 *           the swap-and-pop are made on the device where the status is, and m comes back with the fit's one
 *           read-back, from which the host knows how many words were consumed.
 *   ColorVec (:55).  The first-frame branch draws 3 * nFeatures values uniform(0, 255) from the same generator: a first
 *           frame advances the state by 3 * nFeatures next() calls (hs_twoview_rng_skip).
 *   Median depth (:1283-1297).  Index (size - 1) / 2 of the triangulated z, selected exactly; t and p3d are divided
 *           by it in fp32.  p3d is 0 where the key is not triangulated.
 */
#ifndef HS_TWOVIEW_H
#define HS_TWOVIEW_H

#include "hs_types.h"
#include "hs_flow.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hs_twoview hs_twoview;

#define HS_TWOVIEW_MAX_SETS 256

typedef struct hs_twoview_result {
  int32_t ok;             /* 1: FindTransformation returned true */
  int32_t why;            /* 0 ok; 1 no hypothesis scored above 0; 2 H's singular values too close; 3 no clear winner or
                             too few good points; 4 parallax below minParallax; 5 fewer than 8 matched keys
                             (hs_twoview_fit_flow_drawn only) */
  int32_t model;          /* 0 H, 1 F; -1 when why == 1 */
  int32_t best_h, best_f; /* the winning sets (-1: no set scored above 0) */
  int32_t n_inliers;      /* the chosen model's inliers (N of ReconstructH / ReconstructF) */
  float SH, SF;
  float R[9], t[3];       /* R21 row-major; t21 already divided by the median depth (:142-148); 0 unless ok */
  int32_t n_good;         /* CheckRT's nGood of the winning motion hypothesis */
  float parallax_deg;
  int32_t n_triangulated; /* the keys with vbTriangulated set */
  float median_depth;
  int32_t best_rt;        /* which of the 4 (F) or 8 (H) motion hypotheses won; -1: none */
  int32_t n_rt;           /* the motion hypotheses tested: 0, 4 or 8 */
  int32_t reserved[6];    /* after hs_twoview_fit_flow_drawn: [0], [1] = the low and the high 32 bits of the generator's
                             state behind the call; 0 otherwise */
} hs_twoview_result;      /* 128 bytes */

/* capacity >= 8: the most keys of one fit.  K4 = fx, fy, cx, cy (rounded to fp32: the reference's K is CV_32F). */
int hs_twoview_create(hs_twoview** out, int device_id, int capacity, const double K4[4]);
void hs_twoview_destroy(hs_twoview* tv);

/* The fit from host arrays: xy1[n][2], xy2[n][2], status[n], sets[n_sets][8] (the caller's mvSets).
   HS_ERR_INVALID, the state unchanged: n outside 8 .. capacity; n_sets outside 1 .. 256; an index outside 0 .. n-1 or
   pointing at a key with status 0; two equal indices in one set.  A fit that the reference would refuse is not an
   error: it returns HS_OK with result->ok = 0 and result->why.  *result is nullable. */
int hs_twoview_fit(hs_twoview* tv, int n, const float* xy1, const float* xy2, const uint8_t* status, int n_sets,
                   const int32_t* sets, hs_twoview_result* result);
/* The same with FirstFramePts, MatchedPts and MatchedStatus read where `flow` holds them after its last track, ordered
   behind it with an event; the only read-back is the result record.  The flow must be on this device and hold 8 ..
   capacity keys (HS_ERR_INVALID) after a track (HS_ERR_STATE).  The status rule is checked on the device. */
int hs_twoview_fit_flow(hs_twoview* tv, hs_flow* flow, int n_sets, const int32_t* sets, hs_twoview_result* result);

/* The generator (the contract above).  The state belongs to the context and lives on the host; none of the three
   touches the device.  n_next above 2^30: HS_ERR_INVALID (a skip is a host loop). */
int hs_twoview_rng_seed(hs_twoview* tv, uint64_t seed);
int hs_twoview_rng_skip(hs_twoview* tv, uint64_t n_next);
int hs_twoview_rng_state(hs_twoview* tv, uint64_t* state);
/* Parity entry: the draw alone over a host status[n], made by the kernels of hs_twoview_fit_flow_drawn; advances the
   state; sets_out[n_sets][8]; *m_out (nullable) = the keys with status != 0 as the device counted them.  The last
   fit and its read-backs are not touched.  HS_ERR_INVALID, the state unchanged: n outside 8 .. capacity, n_sets
   outside 1 .. 256, fewer than 8 keys with status != 0. */
int hs_twoview_draw(hs_twoview* tv, int n, const uint8_t* status, int n_sets, int32_t* sets_out, int* m_out);
/* hs_twoview_fit_flow with the sets drawn on the device from the flow's MatchedStatus: no key-sized array and no
   status byte crosses to the host, and the generator's new state comes back in the result record.  With fewer than 8
   matched keys it returns HS_OK with result->ok = 0, why = 5, model, best_h, best_f and best_rt -1 and everything else
   0 but the state words; the state does not move, no kernel of the fit runs, the parity read-backs keep the fit
   before, and hs_refiner_set_points_twoview refuses until the next successful fit. */
int hs_twoview_fit_flow_drawn(hs_twoview* tv, hs_flow* flow, int n_sets, hs_twoview_result* result);
/* The sets of the last fit, drawn or uploaded: sets[n_sets][8].  Before a fit: HS_ERR_STATE. */
int hs_twoview_get_sets(hs_twoview* tv, int32_t* sets);

/* Parity read-backs of the last fit (or debug entry), all nullable: inliers_h[n], inliers_f[n] (the two winners'
   vbMatchesInliers), scores_h[n_sets], scores_f[n_sets], triangulated[n], p3d[n][3] (divided by the median depth),
   models[2][n_sets][9] (H21 of every set, then F21 of every set).  Before a fit: HS_ERR_STATE. */
int hs_twoview_get(hs_twoview* tv, uint8_t* inliers_h, uint8_t* inliers_f, float* scores_h, float* scores_f,
                   uint8_t* triangulated, float* p3d, float* models);
/* The last result record again. */
int hs_twoview_last_result(hs_twoview* tv, hs_twoview_result* result);
/* CheckRT's per-hypothesis outputs of the last fit or hs_twoview_check_rt, all nullable: *n_rt; n_good[n_rt],
   parallax[n_rt]; good[n_rt][n] (vbGood), pass[n_rt][n] (the matches nGood counts), cos_parallax[n_rt][n] (defined
   where pass), p3d[n_rt][n][3] (unscaled; 0 where not pass). */
int hs_twoview_get_rt(hs_twoview* tv, int* n_rt, int32_t* n_good, float* parallax, uint8_t* good, uint8_t* pass,
                      float* cos_parallax, float* p3d);
/* Device time of the last fit's kernels in ms: ms[8] = normalize, hypotheses, scores, winners, decompose, CheckRT,
   select, finish. */
int hs_twoview_last_stats(hs_twoview* tv, double* ms);
/* Device time of the last draw's two kernels (hs_twoview_draw or hs_twoview_fit_flow_drawn) in ms: ms[2] = the list of
   matched keys, the swap-and-pop.  Before a draw: HS_ERR_STATE. */
int hs_twoview_last_draw_stats(hs_twoview* tv, double* ms);

/* Debug entries that split the pipeline at its seams; both work on the keys of the last fit (HS_ERR_STATE before one),
   leave their outputs where hs_twoview_get / _get_rt read them, and end the validity of the last fit for
   hs_refiner_set_points_twoview.
   score_models: only the scoring and the winners' masks, on caller-supplied fp32 matrices H21[n_h][9], H12[n_h][9],
   F21[n_f][9]; n_h, n_f in 1 .. 256.
   check_rt: only the triangulation pass and its select, on caller-supplied motions R[n_rt][9], t[n_rt][3], n_rt in
   1 .. 8, over the matches with inliers[n] != 0. */
int hs_twoview_score_models(hs_twoview* tv, int n_h, const float* H21, const float* H12, int n_f, const float* F21);
int hs_twoview_check_rt(hs_twoview* tv, int n_rt, const float* R, const float* t, const uint8_t* inliers);

#ifdef __cplusplus
}
#endif
#endif /* HS_TWOVIEW_H */
