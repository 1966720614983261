// hs_undist_kernels.h — the fused photometric + geometric undistortion kernel (include/hs_undist.h), its launcher
// and what the pyramid build (hs_image_kernels.h) takes of an undistorter: its tables and its staged frame.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct hs_undistorter;

struct HsUndistArgs {
  int w_in, h_in, n_out;
  int passthrough;      // n_out == w_in * h_in, output pixel i = S(raw[i])
  const uint8_t* raw;   // w_in * h_in
  const int2* map;      // n_out: (cvRound(remap_x * 32), cvRound(remap_y * 32)), fixed at table upload
  const float* Binv;    // 256, null = no gamma
  const float* B;       // 256, null = no photometric tables (img8 = sat8(fImg))
  const float* vinv;    // w_in * h_in, null = no vignette
  float* fimg;          // n_out, nullable
  uint8_t* img8;        // n_out, nullable
};

__global__ void hs_k_undistort(HsUndistArgs a);

// Checks that u is on `device` with a w x h output; HS_ERR_INVALID with hs_last_error set otherwise.
int hs_undist_match(const hs_undistorter* u, int device, int w, int h);
// The tables where they lie on the device: every field of HsUndistArgs but fimg and img8, which are left null.  raw is
// u's own input staging (hs_undist_upload); a caller that stages the frame itself on its own stream (hs_image_set_u8)
// puts its buffer there.  The tables are read-only between hs_undistorter_set_photometric / _set_remap calls, so any
// number of streams may read them.
void hs_undist_tables(const hs_undistorter* u, HsUndistArgs* a);
// Enqueues on `stream` the upload of the raw u8 frame into u's input staging.  The caller synchronises `stream`
// before it returns to its own caller (raw is the user's buffer, and the staging is reused by the next call).
hipError_t hs_undist_upload(hs_undistorter* u, hipStream_t stream, const uint8_t* raw);
// Enqueues on `stream`: hs_undist_upload of raw (null: keep the staged frame), then the kernel into d_fimg
// (w_out*h_out floats, device, nullable) and d_img8 (nullable) -- for a caller that needs the float plane or cvImgL
// without a pyramid; a pyramid is built from the staged frame directly (hs_img_build, hs_image_kernels.h).
hipError_t hs_undist_enqueue(hs_undistorter* u, hipStream_t stream, const uint8_t* raw, float* d_fimg,
                             uint8_t* d_img8);
