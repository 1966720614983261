// hs_undist.cpp — the undistorter context of include/hs_undist.h: the host tables (hs_undist_tables.cpp) placed on
// the device, the standalone apply, and the staging and launcher the other contexts' _u8 entries use.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/hs_ba.h"
#include "../../include/hs_undist.h"
#include "hs_host.h"
#include "hs_undist_kernels.h"
#include "hs_undist_tables.h"

struct hs_undistorter : hs::Device {  // stream: the standalone apply's; e0, e1: hs_undistorter_time_kernel's
  hs::Pool pool;
  int w_in = 0, h_in = 0, w_out = 0, h_out = 0;
  bool passthrough = false;
  float K[4] = {0, 0, 0, 0};
  std::vector<float> rx, ry;  // the table in use, float form (hs_undistorter_get_remap)
  int2* d_map = nullptr;         // (cvRound(x * 32), cvRound(y * 32)) per output pixel
  float *d_Binv = nullptr, *d_B = nullptr, *d_vinv = nullptr;
  bool have_gamma = false, have_vig = false;
  uint8_t* d_in = nullptr;    // staging of the raw frame
  float* d_fimg = nullptr;    // the standalone apply's outputs
  uint8_t* d_img8 = nullptr;
};

// the table to its fixed-point device form; complete on the device at return
static int upload_map(hs_undistorter* u) {
  const size_t n = (size_t)u->w_out * u->h_out;
  std::vector<int2> m(n);
  // cvRound: to nearest, ties to even (the default rounding mode)
  for (size_t i = 0; i < n; i++) m[i] = make_int2((int)std::nearbyint(u->rx[i] * 32.f), (int)std::nearbyint(u->ry[i] * 32.f));
  HS_HIP(hipSetDevice(u->device));
  HS_HIP(hipMemcpy(u->d_map, m.data(), n * sizeof(int2), hipMemcpyHostToDevice));
  return HS_OK;
}

int hs_undist_match(const hs_undistorter* u, int device, int w, int h) {
  if (!u) return hs::fail(HS_ERR_INVALID, "null undistorter");
  if (u->device != device) return hs::fail(HS_ERR_INVALID, "undistorter and consumer are on different devices");
  if (u->w_out != w || u->h_out != h) return hs::fail(HS_ERR_INVALID, "undistorter output size differs from the consumer's");
  return HS_OK;
}

void hs_undist_tables(const hs_undistorter* u, HsUndistArgs* a) {
  a->w_in = u->w_in;
  a->h_in = u->h_in;
  a->n_out = u->w_out * u->h_out;
  a->passthrough = u->passthrough ? 1 : 0;
  a->raw = u->d_in;
  a->map = u->d_map;
  a->Binv = u->have_gamma ? u->d_Binv : nullptr;
  a->B = (u->have_gamma || u->have_vig) ? u->d_B : nullptr;
  a->vinv = u->have_vig ? u->d_vinv : nullptr;
  a->fimg = nullptr;
  a->img8 = nullptr;
}

hipError_t hs_undist_upload(hs_undistorter* u, hipStream_t stream, const uint8_t* raw) {
  return hipMemcpyAsync(u->d_in, raw, (size_t)u->w_in * u->h_in, hipMemcpyHostToDevice, stream);
}

hipError_t hs_undist_enqueue(hs_undistorter* u, hipStream_t stream, const uint8_t* raw, float* d_fimg,
                             uint8_t* d_img8) {
  if (raw) {  // null: the frame already in the staging (the timing loop)
    hipError_t e = hs_undist_upload(u, stream, raw);
    if (e != hipSuccess) return e;
  }
  HsUndistArgs a;
  hs_undist_tables(u, &a);
  a.fimg = d_fimg;
  a.img8 = d_img8;
  hipLaunchKernelGGL(hs_k_undistort, dim3((a.n_out + 255) / 256), dim3(256), 0, stream, a);
  return hipGetLastError();
}

extern "C" {

int hs_undistorter_create(hs_undistorter** out, int device_id, const hs_undist_calib* calib) {
  if (!out) return hs::fail(HS_ERR_INVALID, "null out");
  *out = nullptr;
  if (!calib) return hs::fail(HS_ERR_INVALID, "null calibration");
  if (calib->w_in <= 0 || calib->h_in <= 0 || calib->w_out <= 0 || calib->h_out <= 0 || calib->w_in > 32767 ||
      calib->h_in > 32767 || (long long)calib->w_out * calib->h_out >= (1LL << 30))
    return hs::fail(HS_ERR_INVALID, "bad image size");
  const size_t n_out = (size_t)calib->w_out * calib->h_out, n_in = (size_t)calib->w_in * calib->h_in;
  std::vector<float> rx(n_out), ry(n_out);
  float K[4];
  HS_TRY(hs_undist_make_remap(calib, K, rx.data(), ry.data()));  // the calibration's own checks
  HS_TRY(hs::check_device(device_id));
  hs_undistorter* u = new hs_undistorter();
  u->w_in = calib->w_in;
  u->h_in = calib->h_in;
  u->w_out = calib->w_out;
  u->h_out = calib->h_out;
  for (int i = 0; i < 4; i++) u->K[i] = K[i];
  u->rx = std::move(rx);
  u->ry = std::move(ry);
  u->passthrough = calib->process == HS_UNDIST_NONE;
  int rc = [&]() -> int {
    hs::Pool& m = u->pool;
    if (u->open(device_id) || m.alloc(&u->d_map, n_out) || m.alloc(&u->d_Binv, 256) || m.alloc(&u->d_B, 256) ||
        m.alloc(&u->d_vinv, n_in) || m.alloc(&u->d_in, n_in) || m.alloc(&u->d_fimg, n_out) ||
        m.alloc(&u->d_img8, n_out))
      return hs::fail(HS_ERR_NOMEM, "undistorter allocation failed");
    return upload_map(u);
  }();
  if (rc) hs_undistorter_destroy(u);
  else *out = u;
  return rc;
}

void hs_undistorter_destroy(hs_undistorter* u) {
  if (!u) return;
  (void)hipSetDevice(u->device);
  if (u->stream) (void)hipStreamSynchronize(u->stream);
  u->pool.release_all();
  u->close();
  delete u;
}

int hs_undistorter_set_photometric(hs_undistorter* u, const float* G256, const uint16_t* vignette) {
  if (!u) return hs::fail(HS_ERR_INVALID, "null undistorter");
  const size_t n_in = (size_t)u->w_in * u->h_in;
  float Binv[256], B[256];
  std::vector<float> vinv(vignette ? n_in : 0);
  int rc = hs_undist_make_photometric(G256, vignette, (int)n_in, Binv, B, vignette ? vinv.data() : nullptr);
  if (rc) return rc;
  HS_HIP(hipSetDevice(u->device));
  HS_HIP(hipMemcpy(u->d_Binv, Binv, sizeof(Binv), hipMemcpyHostToDevice));
  HS_HIP(hipMemcpy(u->d_B, B, sizeof(B), hipMemcpyHostToDevice));
  if (vignette) HS_HIP(hipMemcpy(u->d_vinv, vinv.data(), n_in * sizeof(float), hipMemcpyHostToDevice));
  u->have_gamma = G256 != nullptr;
  u->have_vig = vignette != nullptr;
  return HS_OK;
}

int hs_undistorter_set_remap(hs_undistorter* u, const float* remap_x, const float* remap_y) {
  if (!u || !remap_x || !remap_y) return hs::fail(HS_ERR_INVALID, "null argument");
  const size_t n = (size_t)u->w_out * u->h_out;
  int rc = hs_undist_check_map(remap_x, remap_y, n);
  if (rc) return rc;
  u->rx.assign(remap_x, remap_x + n);
  u->ry.assign(remap_y, remap_y + n);
  u->passthrough = false;
  return upload_map(u);
}

int hs_undistorter_get_K(const hs_undistorter* u, float K_out[4]) {
  if (!u || !K_out) return hs::fail(HS_ERR_INVALID, "null argument");
  for (int i = 0; i < 4; i++) K_out[i] = u->K[i];
  return HS_OK;
}

int hs_undistorter_get_remap(const hs_undistorter* u, float* remap_x, float* remap_y) {
  if (!u) return hs::fail(HS_ERR_INVALID, "null undistorter");
  const size_t n = (size_t)u->w_out * u->h_out;
  for (size_t i = 0; i < n; i++) {
    if (remap_x) remap_x[i] = u->rx[i];
    if (remap_y) remap_y[i] = u->ry[i];
  }
  return HS_OK;
}

int hs_undistorter_apply(hs_undistorter* u, const uint8_t* raw, float* fimg_out, uint8_t* img8_out) {
  if (!u || !raw) return hs::fail(HS_ERR_INVALID, "null argument");
  const size_t n = (size_t)u->w_out * u->h_out;
  HS_HIP(hipSetDevice(u->device));
  hipError_t e = hs_undist_enqueue(u, u->stream, raw, fimg_out ? u->d_fimg : nullptr, img8_out ? u->d_img8 : nullptr);
  if (e == hipSuccess && fimg_out)
    e = hipMemcpyAsync(fimg_out, u->d_fimg, n * sizeof(float), hipMemcpyDeviceToHost, u->stream);
  if (e == hipSuccess && img8_out) e = hipMemcpyAsync(img8_out, u->d_img8, n, hipMemcpyDeviceToHost, u->stream);
  const hipError_t es = hipStreamSynchronize(u->stream);  // also after a failure: the caller's buffers are in flight
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return hs::fail(HS_ERR_HIP, std::string("hs_undistorter_apply: ") + hipGetErrorString(e));
  return HS_OK;
}

int hs_undistorter_time_kernel(hs_undistorter* u, const uint8_t* raw, int warmup, int launches, float* ms_per_launch) {
  if (!u || !raw || !ms_per_launch) return hs::fail(HS_ERR_INVALID, "null argument");
  if (warmup < 0 || launches < 1) return hs::fail(HS_ERR_INVALID, "bad launch count");
  HS_HIP(hipSetDevice(u->device));
  const hipEvent_t e0 = u->e0, e1 = u->e1;
  int rc = HS_OK;
  hipError_t e = hipMemcpyAsync(u->d_in, raw, (size_t)u->w_in * u->h_in, hipMemcpyHostToDevice, u->stream);
  for (int i = 0; i < warmup + launches && e == hipSuccess; i++) {
    if (i == warmup) e = hipEventRecord(e0, u->stream);
    if (e == hipSuccess) e = hs_undist_enqueue(u, u->stream, nullptr, u->d_fimg, nullptr);
  }
  if (e == hipSuccess) e = hipEventRecord(e1, u->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(u->stream);
  float ms = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  if (e != hipSuccess) rc = hs::fail(HS_ERR_HIP, std::string("hs_undistorter_time_kernel: ") + hipGetErrorString(e));
  *ms_per_launch = ms / (float)launches;
  return rc;
}

}  // extern "C"
