// hs_extract_kernels.h — kernels of include/hs_extract.h (blur, ordered key compaction, angle + descriptor) and the
// hand-off the tracer reads the keys through.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct hs_extractor;

constexpr int kExtBorder = 19;        // HALF_PATCH_SIZE + 4: keys lie in [19, W-19) x [19, H-19)
constexpr int kExtHalfPatch = 15;     // IC_Angle's disc
constexpr int kExtPatternMax = 13;    // |pattern entry| <= 13: a rotated tap reaches rint(13 * sqrt(2)) = 18 px
constexpr int kExtBlurTileW = 64, kExtBlurTileH = 16;  // one 256-thread block, 4 pixels of a row per thread

// 7x7 separable fixed-point Gaussian, u8 -> u8, reflect-101 (include/hs_extract.h)
struct HsExtBlurArgs {
  int W, H;
  int w[4];            // weights of taps 0..3 (outer .. centre); taps 4..6 mirror 2..0
  const uint8_t* src;  // W*H
  uint8_t* dst;        // W*H
};

// the map's interior compacted in raster order
struct HsExtKeysArgs {
  int W, H, cap;
  const float* map;  // W*H
  int* row_cnt;      // [H - 38] keys per interior row
  float* x;          // [cap]
  float* y;          // [cap]
  int* count;        // keys found (also when > cap: nothing is written then)
};

struct HsExtDescArgs {
  int W, cap;
  unsigned long long umax;  // umax[0..15], 4 bits each: a register shift, where an indexed table would go to memory
  const int* count;
  const float* x;
  const float* y;
  const uint8_t* img;      // unblurred
  const uint8_t* blurred;
  const char4* pattern;    // [256] (p.x, p.y, q.x, q.y)
  float* angle;            // [cap]
  uint32_t* desc;          // [cap][8]
};

__global__ void hs_k_ext_blur(HsExtBlurArgs a);
__global__ void hs_k_ext_count(HsExtKeysArgs a);
__global__ void hs_k_ext_write(HsExtKeysArgs a);
__global__ void hs_k_ext_desc(HsExtDescArgs a);

// The last successful extract's keys where they lie on the device (x / y: n floats each, raster order), and the
// event on the extractor's stream after which they are complete: a consumer's stream waits on it before it reads.
void hs_extract_keys(hs_extractor* e, int* device, int* W, int* H, int* n, const float** d_x, const float** d_y,
                     hipEvent_t* ready);
// Called by the consumer after it has enqueued its reads on `consumer`: the extractor's next extract waits for them
// before it reuses the buffers.
hipError_t hs_extract_keys_consumed(hs_extractor* e, hipStream_t consumer);
// cvImgL (W*H bytes) where the last extract put it on the device, and the event after which it is complete (the
// extract's closing event: the same as the keys').  The image is that of the last extract call, also of one that
// overflowed; the next extract overwrites it, so a consumer waits for its own reads before it returns.  False before
// the first extract: there is no image yet.
bool hs_extract_image(hs_extractor* e, int* device, int* W, int* H, const uint8_t** d_img, hipEvent_t* ready);
