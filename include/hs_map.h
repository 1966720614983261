/*
 * hs_map.h — the device-resident map of the points that left the BA window, and the frame decision that needs its
 * counters.  Plain C, the conventions of hs_ba.h: status codes, caller-owned host buffers, no allocation after
 * hs_map_create.
 *
 * Reference interface each entry point replaces (AUBVRL/H-SLAM):
 *   hs_map_create / hs_map_destroy      Frame::pointHessiansMarginalized / pointHessiansOut of every keyframe
 *                                       (Src/Mapping.cpp:272,300,306,313; Src/FullSystemOptimize.cpp:589): one
 *                                       append-only store of fixed capacity on the device.
 *   hs_ba_attach_map                    (new) the window's removals append to the map before the points leave.
 *   hs_map_retire_points                the same push for a caller that decides itself (before hs_ba_remove_points).
 *   hs_map_frame_counts                 pointHessiansMarginalized.size() / pointHessiansOut.size()
 *                                       (Src/FullSystemMarginalize.cpp:36-37).
 *   hs_map_refresh_cloud                KFDisplay::RefreshPC for one keyframe (Src/Display.cpp:382-513).
 *   hs_ba_flag_frames_for_marginalization   System::flagFramesForMarginalization
 *                                       (Src/FullSystemMarginalize.cpp:18-103).
 */
#ifndef HS_MAP_H
#define HS_MAP_H

#include "hs_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hs_map hs_map;

/* the reference's PtStatus values a retired point can have (Include/MapPoint.h) */
enum { HS_PT_OUTLIER = 1, HS_PT_MARGINALIZED = 3 };

/* One retired point: 64 bytes, four 16-byte quarters (the retire kernel stores one quarter per lane).  Every value is
   the window's device state at the moment the point left: idepth, idepth_zero, maxRelBaseline, numGoodResiduals and
   hdif (the last solve's HdiF) exactly as hs_ba_get_point_state returns them; idepth_hessian = hdif > 0 ? 1 / hdif : 0
   in fp64 (the convention of hs_ba_flag_points_for_removal).  color: the eight pattern colours converted to unsigned
   char the way the reference's display converts them, Vec3b(color[k], ...) (truncation toward zero; the window keeps
   them as floats in [0, 255]) -- the only reader of a retired MapPoint's colours is KFDisplay::RefreshPC. */
typedef struct hs_map_record {
  int32_t handle;            /* the point's window handle (hs_ba_insert_points) */
  int32_t frame_id;          /* the host keyframe's hs_frame.id */
  int32_t status;            /* HS_PT_OUTLIER or HS_PT_MARGINALIZED */
  int32_t numGoodResiduals;
  float u, v, idepth, idepth_zero;
  float hdif, maxRelBaseline;
  uint8_t color[8];
  uint8_t reserved[16];      /* zero */
} hs_map_record;

/* An empty map for capacity_points records on device_id. */
int hs_map_create(hs_map** out, int capacity_points, int device_id);
void hs_map_destroy(hs_map* map);

/* Attach `map` to the context (NULL detaches); a context has at most one map, a map serves one context at a time.
   Single-rank contexts only (HS_ERR_STATE with a communicator or in a rank group); the map must live on the context's
   device (HS_ERR_INVALID).  Without an attached map every call of hs_ba.h behaves exactly as it does without this
   header, including which calls commit and when.  With one:
     hs_ba_flag_points_for_removal(apply = 1)   appends every action != 0 point of the committed window in window order
         (the reference's push order: frames in window order, each frame's pointHessians in list order), action 1 as
         HS_PT_OUTLIER, action 2 as HS_PT_MARGINALIZED, from the device state the decision just read, after the
         decision kernel and before the marginalization pass and the removals; nothing more is read back.
     hs_ba_remove_points_without_residuals      appends the removed points in removal order as HS_PT_OUTLIER.  The
         records are copies of the points' committed device state, so the call commits pending edits first when one of
         the leaving points has been inserted since the last commit (without a map it never commits).
   A retire that would exceed the map's capacity returns HS_ERR_NOMEM before the window or the map has changed.
   Detach (or destroy the context) before hs_map_destroy. */
int hs_ba_attach_map(hs_ctx* ctx, hs_map* map);

/* Append n points of ctx's committed window (by handle, in the given order) to the attached map with the given
   status each, for a caller that decides itself; call it before hs_ba_remove_points.  Commits first.  A handle that is
   not in the committed window, or a status other than HS_PT_OUTLIER / HS_PT_MARGINALIZED, returns HS_ERR_INVALID and
   appends nothing; no attached map: HS_ERR_STATE. */
int hs_map_retire_points(hs_ctx* ctx, int n, const int* handles, const uint8_t* status);

/* records stored, and keyframes (distinct frame_id) that have at least one (both nullable) */
int hs_map_size(hs_map* map, int* n_records, int* n_frames);
/* the frame's pointHessiansMarginalized.size() and pointHessiansOut.size(); host-side counters, no device work;
   a frame_id the map has never seen gives 0 / 0 (both nullable) */
int hs_map_frame_counts(hs_map* map, int frame_id, int* n_marginalized, int* n_out);
/* records [first, first + n) in push order into out[n] */
int hs_map_get_records(hs_map* map, int first, int n, hs_map_record* out);
/* forget every record (the capacity stays) */
int hs_map_clear(hs_map* map);

/* KFDisplay::RefreshPC (Src/Display.cpp:382-513) for the keyframe frame_id: the frame's active points, if it is
   still in ctx's committed window (commits first), in window order, then its HS_PT_MARGINALIZED records in push
   order.  Per point: skipped if idepth < 0; depth = 1.0f / idepth; depth4 = (depth * depth)^2;
   var = (float)(1.0 / ((double)idepth_hessian + 0.01)); skipped if var * depth4 > 0.001f, var > 0.001f or
   maxRelBaseline < 0.1f.  A kept point emits its 8 pattern pixels: x = ((u + dx) * fxi + cxi) * depth, y likewise
   (fp32, no contraction), z = depth; colour (0, 0, 255) for active points, (c, c, c) of the record's colour for
   marginalized ones.  The reference's z jitter (depth * 2 * fxi * (rand() / RAND_MAX - 0.5), process-global rand()
   state) is not applied.
     xyz_out [cap][3] float, rgb_out [cap][3] uint8 (nullable): the first min(n, cap) vertices; n_out: the vertex count
     (8 per kept point); kinv_out[4] (nullable): the fxi, fyi, cxi, cyi the kernel used (the window's current
     calibration).
   More vertices than the map can hold (8 * capacity_points) return HS_ERR_NOMEM.  The vertices and colours stay in
   device buffers owned by the map (hs_map_cloud_device) until the next refresh. */
int hs_map_refresh_cloud(hs_map* map, hs_ctx* ctx, int frame_id, float* xyz_out, uint8_t* rgb_out, int cap, int* n_out,
                         float* kinv_out);
/* device addresses of the last refresh's vertices ([n][3] float) and colours ([n][3] uint8), and n (all nullable);
   the refresh has completed when hs_map_refresh_cloud returned */
int hs_map_cloud_device(hs_map* map, const float** d_xyz, const uint8_t** d_rgb, int* n);

/* System::flagFramesForMarginalization's settings (Src/Settings.cpp:52-59) */
typedef struct hs_frame_marg_params {
  int minFrameAge;              /* setting_minFrameAge 1 */
  int maxFrames;                /* setting_maxFrames 7 */
  int minFrames;                /* setting_minFrames 5 */
  float minPointsRemaining;     /* setting_minPointsRemaining 0.05 */
  float maxLogAffFacInWindow;   /* setting_maxLogAffFacInWindow 0.7 */
} hs_frame_marg_params;
int hs_frame_marg_params_default(hs_frame_marg_params* out);

/* System::flagFramesForMarginalization (Src/FullSystemMarginalize.cpp:18-103) on the committed window (commits first).
   Per window frame f: in = the active points it hosts + n_immature[f] (the caller's tracer; nullable => 0), out = the
   attached map's two counters for its hs_frame.id, the affine factor from the newest frame (exposures and the current
   aff_g2l), the pair distances |(T.PRE_worldToCam * H.PRE_camToWorld).translation()| and kf_id[f] (KfId).  The factors
   and distances are formed on the device from the window's frame state and the rule runs there; only the nF flag
   bytes are read back.  flagged_out[nF]: 1 = FlaggedForMarginalization by this call; n_flagged nullable.
   Deviation: where no frame passes the age test the reference dereferences an empty toMarginalize; the call flags
   nothing more and returns HS_OK.
   Requires an attached map (HS_ERR_STATE otherwise; single-rank contexts, as hs_ba_attach_map). */
int hs_ba_flag_frames_for_marginalization(hs_ctx* ctx, const hs_frame_marg_params* params, const int* kf_id,
                                          const int* n_immature, uint8_t* flagged_out, int* n_flagged);

#ifdef __cplusplus
}
#endif
#endif /* HS_MAP_H */
