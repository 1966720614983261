// hs_pyr.cpp — the standalone C-ABI entry of the device image pyramid (include/hs_pyr.h).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/hs_ba.h"
#include "../../include/hs_pyr.h"
#include "hs_host.h"
#include "hs_image_kernels.h"

// the body of hs_dir_pyramid; the caller waits for the stream and frees `scratch` on every path
static int dir_pyramid(hs::Device& dev, hs::Pool& scratch, int device_id, int width, int height, int n_levels,
                       const float* img, float* dirpyr_out, float* abs_squared_grad_out) {
  float* d_img = nullptr;
  float4* lv[HS_MAX_LEVELS] = {nullptr};
  float* ag[HS_MAX_LEVELS] = {nullptr};
  HS_TRY(dev.open(device_id));
  const hipStream_t s = dev.stream;
  HS_TRY(scratch.alloc(&d_img, (size_t)width * height));
  for (int l = 0; l < n_levels; l++) {
    const size_t n = (size_t)(width >> l) * (height >> l);
    HS_TRY(scratch.alloc(&lv[l], n));
    HS_TRY(scratch.alloc(&ag[l], n));
  }
  HS_HIP(hipMemcpyAsync(d_img, img, sizeof(float) * width * height, hipMemcpyHostToDevice, s));
  HS_HIP(hs_img_build(s, width, height, n_levels, lv, ag, nullptr, d_img, nullptr));
  size_t off3 = 0, off1 = 0;
  std::vector<float4> tex;
  for (int l = 0; l < n_levels; l++) {
    const size_t n = (size_t)(width >> l) * (height >> l);
    tex.resize(n);
    HS_HIP(hipMemcpyAsync(tex.data(), lv[l], n * sizeof(float4), hipMemcpyDeviceToHost, s));
    if (abs_squared_grad_out)
      HS_HIP(hipMemcpyAsync(abs_squared_grad_out + off1, ag[l], n * sizeof(float), hipMemcpyDeviceToHost, s));
    HS_HIP(hipStreamSynchronize(s));
    if (dirpyr_out)
      for (size_t i = 0; i < n; i++) {
        dirpyr_out[off3 + 3 * i] = tex[i].x;
        dirpyr_out[off3 + 3 * i + 1] = tex[i].y;
        dirpyr_out[off3 + 3 * i + 2] = tex[i].z;
      }
    off3 += 3 * n;
    off1 += n;
  }
  return HS_OK;
}

extern "C" int hs_dir_pyramid(int device_id, int width, int height, int n_levels, const float* img, float* dirpyr_out,
                              float* abs_squared_grad_out) {
  if (!img) return hs::fail(HS_ERR_INVALID, "null image");
  if (n_levels < 1 || n_levels > HS_MAX_LEVELS || width < 4 || height < 4 || (width >> (n_levels - 1)) < 2 ||
      (height >> (n_levels - 1)) < 2)
    return hs::fail(HS_ERR_INVALID, "bad pyramid size");
  HS_TRY(hs::check_device(device_id));
  hs::Device dev;
  hs::Pool scratch;
  const int rc = dir_pyramid(dev, scratch, device_id, width, height, n_levels, img, dirpyr_out, abs_squared_grad_out);
  if (dev.stream) (void)hipStreamSynchronize(dev.stream);
  scratch.release_all();
  dev.close();
  return rc;
}
