// hs_image_kernels.h — the two kernels behind hs_image_set_* (include/hs_image.h), and what the consumers' entries
// read of an image: its levels where they lie on the device, the event that says they are complete and the event
// a consumer leaves behind for the image's next set.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/hs_types.h"

struct hs_image;

constexpr int kImgTile = 32;      // level-0 tile side: a multiple of 2^(HS_MAX_LEVELS - 1), so every fold stays in the tile
constexpr int kImgThreads = 256;  // 8 rows of the tile per pass, 4 passes

struct HsImgLevelsArgs {
  int W, H, nlev;
  int w_in, h_in;       // the camera frame (u8 path)
  int passthrough;      // output pixel i = S(raw[i])
  const float* fimg;    // W*H floats: the float path (a plain load); null = the u8 path below
  const uint8_t* raw;   // w_in * h_in
  const int2* map;      // W*H: the undistorter's fixed-point table
  const float* Binv;    // 256, null = no gamma
  const float* B;       // 256, null = no photometric tables
  const float* vinv;    // w_in * h_in, null = no vignette
  float4* lvl[HS_MAX_LEVELS];
  uint8_t* img8;        // W*H, null on the float path
};

struct HsImgGradsArgs {
  int nlev;
  int boff[HS_MAX_LEVELS + 1];  // first block of each level; boff[nlev] = the grid
  int w[HS_MAX_LEVELS], h[HS_MAX_LEVELS];
  float4* lvl[HS_MAX_LEVELS];
  float* absg[HS_MAX_LEVELS];
};

__global__ void hs_k_img_levels(HsImgLevelsArgs a);
__global__ void hs_k_img_grads(HsImgGradsArgs a);

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
