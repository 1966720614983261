// hs_image_kernels.h — the library's pyramid build: its two kernels and the launcher every host file calls
// (hs_img_build); and what the consumers' entries read of a device image (include/hs_image.h): its levels where they
// lie on the device, the event that says they are complete and the event a consumer leaves behind for the image's
// next set.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/hs_types.h"
#include "hs_undist_kernels.h"

struct hs_image;

constexpr int kImgTile = 32;      // level-0 tile side: a multiple of 2^(HS_MAX_LEVELS - 1), so every fold stays in the tile
constexpr int kImgThreads = 256;  // 8 rows of the tile per pass, 4 passes

struct HsImgLevelsArgs {
  int W, H, nlev;
  int w_in, h_in;       // the camera frame (u8 source)
  int passthrough;      // output pixel i = S(raw[i])
  // level 0's source: fimg, else raw with the tables below, else (both null) the texels already in lvl[0]
  const float* fimg;    // W*H floats (a plain load)
  const uint8_t* raw;   // w_in * h_in
  const int2* map;      // W*H: the undistorter's fixed-point table
  const float* Binv;    // 256, null = no gamma
  const float* B;       // 256, null = no photometric tables
  const float* vinv;    // w_in * h_in, null = no vignette
  float4* lvl[HS_MAX_LEVELS];
  uint8_t* img8;        // W*H, nullable; written from the u8 source only
};

struct HsImgGradsArgs {
  int nlev;
  int boff[HS_MAX_LEVELS + 1];  // first block of each level; a level without blocks (w = h = 0) is skipped
  int w[HS_MAX_LEVELS], h[HS_MAX_LEVELS];
  float4* lvl[HS_MAX_LEVELS];
  float* absg[HS_MAX_LEVELS];   // entries nullable
};

__global__ void hs_k_img_levels(HsImgLevelsArgs a);
__global__ void hs_k_img_grads(HsImgGradsArgs a);

// Enqueues on `stream` the build of levels 0 .. nlev-1 (sizes W >> l, H >> l) of a frame's direct pyramid into lvl[l]
// (float4 texels), absSquaredGrad into absg[l] (the array or single entries may be null) and, from a u8 source, cvImgL
// into img8 (nullable).  Level 0 comes from one of three sources:
//   fimg            a float plane on the device (W*H);
//   u8 (fimg null)  a raw u8 frame on the device and an undistorter's tables (hs_undist_tables; u8->raw is the frame);
//   both null       lvl[0]'s texels as they are: their intensities are read, level 0 is not written (its gradients
//                   are the owner's), and levels 1 .. nlev-1 are built.
// Two launches, or none where nothing is to build (level 0 in place and nlev == 1).  Returns the first launch error.
hipError_t hs_img_build(hipStream_t stream, int W, int H, int nlev, float4* const* lvl, float* const* absg,
                        uint8_t* img8, const float* fimg, const HsUndistArgs* u8);

// What a consumer's entry takes from an image after the checks every entry shares: the image is on `device`, of size
// w x h, has at least `min_levels` levels (HS_ERR_INVALID otherwise), holds a frame and, where `need_img8`, a cvImgL
// (HS_ERR_STATE otherwise).  No device call.
struct HsImageView {
  float4* const* lvl;   // DirPyr[l] texels
  float* const* absg;   // absSquaredGrad[l]
  const uint8_t* img8;  // cvImgL (null after hs_image_set_raw)
  hipEvent_t ready;     // the last set's kernels
};
int hs_image_view(hs_image* im, int device, int w, int h, int min_levels, bool need_img8, HsImageView* v);
// Records the consumer's reads (its device-to-device copies, enqueued on `consumer`) for the image's next set to
// wait on before it overwrites the levels.
hipError_t hs_image_consumed(hs_image* im, hipStream_t consumer);
