// hs_image.cpp — the launcher of the library's pyramid build (hs_img_build: the image's sets and every context's own
// frame go through it), and the image context of include/hs_image.h: argument checks, the staging of the raw frame,
// one set as an upload and two launches on the image's stream, and the two events that order it with its consumers
// (the consumers' entries live in each consumer's own .cpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/hs_ba.h"
#include "../../include/hs_image.h"
#include "hs_host.h"
#include "hs_image_kernels.h"
#include "hs_undist_kernels.h"

struct hs_image : hs::Device {  // e0, e1: the last set's first and last kernel; e1 is also its "ready" event
  hs::Pool pool;
  int W = 0, H = 0, nlev = 0;
  float4* d_lvl[HS_MAX_LEVELS] = {nullptr};   // DirPyr[l]
  float* d_absg[HS_MAX_LEVELS] = {nullptr};   // absSquaredGrad[l]
  uint8_t* d_img8 = nullptr;                  // cvImgL
  // staging of the caller's frame: pinned on the host (a set returns before its upload ran), then on the device;
  // the undistorter's own d_in belongs to the stream of whoever calls hs_undist_upload
  uint8_t *h_raw = nullptr, *d_raw = nullptr;
  size_t raw_cap = 0;
  float *h_fimg = nullptr, *d_fimg = nullptr;
  hipEvent_t ev_upload = nullptr;  // the last upload from h_raw / h_fimg: waited on before the host rewrites them
  bool upload_pending = false;
  bool have = false, have_img8 = false;
  // one event per consumer entry since the last set (hs_image_consumed); `spare` are recycled ones
  std::vector<hipEvent_t> pending, spare;
};

namespace {

// what every set starts with: the staging is the host's again, and the levels are nobody's
int begin_set(hs_image* im) {
  HS_HIP(hipSetDevice(im->device));
  if (im->upload_pending) {
    HS_HIP(hipEventSynchronize(im->ev_upload));  // an upload: short, and as a rule long done
    im->upload_pending = false;
  }
  for (hipEvent_t ev : im->pending) {
    HS_HIP(hipStreamWaitEvent(im->stream, ev, 0));
    im->spare.push_back(ev);
  }
  im->pending.clear();
  return HS_OK;
}

// the build of every level from the staged frame (fimg, or u8 with its tables), between the timing events
int run_set(hs_image* im, uint8_t* img8, const float* fimg, const HsUndistArgs* u8) {
  HS_HIP(hipEventRecord(im->e0, im->stream));
  HS_HIP(hs_img_build(im->stream, im->W, im->H, im->nlev, im->d_lvl, im->d_absg, img8, fimg, u8));
  HS_HIP(hipEventRecord(im->e1, im->stream));
  return HS_OK;
}

}  // namespace

hipError_t hs_img_build(hipStream_t stream, int W, int H, int nlev, float4* const* lvl, float* const* absg,
                        uint8_t* img8, const float* fimg, const HsUndistArgs* u8) {
  const int first = (fimg || u8) ? 0 : 1;  // the first level whose gradients are formed here
  if (first >= nlev) return hipSuccess;
  HsImgLevelsArgs a;
  a.W = W;
  a.H = H;
  a.nlev = nlev;
  a.w_in = u8 ? u8->w_in : 0;
  a.h_in = u8 ? u8->h_in : 0;
  a.passthrough = u8 ? u8->passthrough : 0;
  a.fimg = fimg;
  a.raw = (u8 && !fimg) ? u8->raw : nullptr;
  a.map = u8 ? u8->map : nullptr;
  a.Binv = u8 ? u8->Binv : nullptr;
  a.B = u8 ? u8->B : nullptr;
  a.vinv = u8 ? u8->vinv : nullptr;
  a.img8 = a.raw ? img8 : nullptr;
  HsImgGradsArgs g;
  g.nlev = nlev;
  int blocks = 0;
  for (int l = 0; l < HS_MAX_LEVELS; l++) {
    const bool on = l < nlev;
    a.lvl[l] = on ? lvl[l] : nullptr;
    g.lvl[l] = a.lvl[l];
    g.absg[l] = (on && absg) ? absg[l] : nullptr;
    g.w[l] = (on && l >= first) ? W >> l : 0;  // a level below `first` gets no blocks
    g.h[l] = (on && l >= first) ? H >> l : 0;
    g.boff[l] = blocks;
    blocks += (g.w[l] * g.h[l] + 255) / 256;
  }
  g.boff[HS_MAX_LEVELS] = blocks;
  hipLaunchKernelGGL(hs_k_img_levels, dim3((W + kImgTile - 1) / kImgTile, (H + kImgTile - 1) / kImgTile),
                     dim3(kImgThreads), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hs_k_img_grads, dim3(blocks), dim3(256), 0, stream, g);
  return hipGetLastError();
}

int hs_image_view(hs_image* im, int device, int w, int h, int min_levels, bool need_img8, HsImageView* v) {
  if (!im) return hs::fail(HS_ERR_INVALID, "null image");
  if (im->device != device) return hs::fail(HS_ERR_INVALID, "image and consumer are on different devices");
  if (im->W != w || im->H != h) return hs::fail(HS_ERR_INVALID, "image size differs from the consumer's");
  if (im->nlev < min_levels)
    return hs::fail(HS_ERR_INVALID, "the image has " + std::to_string(im->nlev) + " levels, the consumer reads " +
                                        std::to_string(min_levels));
  if (!im->have) return hs::fail(HS_ERR_STATE, "the image holds no frame (hs_image_set_u8 / hs_image_set_raw)");
  if (need_img8 && !im->have_img8)
    return hs::fail(HS_ERR_STATE, "the image holds no cvImgL: its frame came from hs_image_set_raw");
  v->lvl = im->d_lvl;
  v->absg = im->d_absg;
  v->img8 = im->have_img8 ? im->d_img8 : nullptr;
  v->ready = im->e1;
  return HS_OK;
}

hipError_t hs_image_consumed(hs_image* im, hipStream_t consumer) {
  hipEvent_t ev = nullptr;
  if (!im->spare.empty()) {
    ev = im->spare.back();
    im->spare.pop_back();
  } else {
    const hipError_t rc = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (rc != hipSuccess) return rc;
  }
  const hipError_t rc = hipEventRecord(ev, consumer);
  if (rc == hipSuccess) im->pending.push_back(ev);
  else im->spare.push_back(ev);
  return rc;
}

extern "C" {

int hs_image_create(hs_image** out, int device_id, int width, int height, int n_levels) {
  if (!out) return hs::fail(HS_ERR_INVALID, "null out");
  *out = nullptr;
  if (n_levels < 1 || n_levels > HS_MAX_LEVELS) return hs::fail(HS_ERR_INVALID, "n_levels out of range");
  if (width < 1 || height < 1) return hs::fail(HS_ERR_INVALID, "image side < 1");
  if ((width >> (n_levels - 1)) < 1 || (height >> (n_levels - 1)) < 1)
    return hs::fail(HS_ERR_INVALID, "image too small for the pyramid: its top level would be empty");
  if ((long long)width * height >= (1LL << 30)) return hs::fail(HS_ERR_INVALID, "image too large");
  HS_TRY(hs::check_device(device_id));
  hs_image* im = new hs_image();
  im->W = width;
  im->H = height;
  im->nlev = n_levels;
  const int rc = [&]() -> int {
    hs::Pool& m = im->pool;
    HS_TRY(im->open(device_id));
    HS_HIP(hipEventCreateWithFlags(&im->ev_upload, hipEventDisableTiming));
    for (int l = 0; l < n_levels; l++) {
      const size_t n = (size_t)(width >> l) * (height >> l);
      HS_TRY(m.alloc(&im->d_lvl[l], n));
      HS_TRY(m.alloc(&im->d_absg[l], n));
    }
    HS_TRY(m.alloc(&im->d_img8, (size_t)width * height));
    return HS_OK;
  }();
  if (rc) hs_image_destroy(im);
  else *out = im;
  return rc;
}

void hs_image_destroy(hs_image* im) {
  if (!im) return;
  (void)hipSetDevice(im->device);
  if (im->stream) (void)hipStreamSynchronize(im->stream);
  for (hipEvent_t ev : im->pending) (void)hipEventSynchronize(ev);  // a consumer may still be copying a level
  im->pool.release_all();
  for (hipEvent_t ev : im->pending) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : im->spare) (void)hipEventDestroy(ev);
  if (im->ev_upload) (void)hipEventDestroy(im->ev_upload);
  im->close();
  delete im;
}

int hs_image_set_u8(hs_image* im, hs_undistorter* u, const uint8_t* raw) {
  if (!im || !u || !raw) return hs::fail(HS_ERR_INVALID, "null argument");
  HS_TRY(hs_undist_match(u, im->device, im->W, im->H));
  HsUndistArgs t;
  hs_undist_tables(u, &t);
  const size_t n_in = (size_t)t.w_in * t.h_in;
  HS_TRY(begin_set(im));
  if (n_in > im->raw_cap) {  // the first set, or an undistorter of a larger camera frame
    HS_HIP(hipStreamSynchronize(im->stream));
    im->raw_cap = 0;
    HS_TRY(im->pool.pinned(&im->h_raw, n_in));
    HS_TRY(im->pool.alloc(&im->d_raw, n_in));
    im->raw_cap = n_in;
  }
  std::memcpy(im->h_raw, raw, n_in);
  HS_HIP(hipMemcpyAsync(im->d_raw, im->h_raw, n_in, hipMemcpyHostToDevice, im->stream));
  HS_HIP(hipEventRecord(im->ev_upload, im->stream));
  im->upload_pending = true;
  t.raw = im->d_raw;  // the image's own staging, on its own stream
  im->have = im->have_img8 = false;  // until the launches are enqueued
  HS_TRY(run_set(im, im->d_img8, nullptr, &t));
  im->have = im->have_img8 = true;
  return HS_OK;
}

int hs_image_set_raw(hs_image* im, const float* fimg) {
  if (!im || !fimg) return hs::fail(HS_ERR_INVALID, "null argument");
  const size_t n = (size_t)im->W * im->H;
  HS_TRY(begin_set(im));
  if (!im->d_fimg) {
    HS_TRY(im->pool.pinned(&im->h_fimg, n));
    HS_TRY(im->pool.alloc(&im->d_fimg, n));
  }
  std::memcpy(im->h_fimg, fimg, n * sizeof(float));
  HS_HIP(hipMemcpyAsync(im->d_fimg, im->h_fimg, n * sizeof(float), hipMemcpyHostToDevice, im->stream));
  HS_HIP(hipEventRecord(im->ev_upload, im->stream));
  im->upload_pending = true;
  im->have = im->have_img8 = false;
  HS_TRY(run_set(im, nullptr, im->d_fimg, nullptr));
  im->have = true;
  return HS_OK;
}

int hs_image_get(hs_image* im, int lvl, float* dirpyr_out, float* absg_out, uint8_t* img8_out) {
  if (!im) return hs::fail(HS_ERR_INVALID, "null image");
  if (lvl < 0 || lvl >= im->nlev) return hs::fail(HS_ERR_INVALID, "bad level");
  if (img8_out && lvl != 0) return hs::fail(HS_ERR_INVALID, "cvImgL exists at level 0 only");
  if (!im->have) return hs::fail(HS_ERR_STATE, "the image holds no frame (hs_image_set_u8 / hs_image_set_raw)");
  if (img8_out && !im->have_img8)
    return hs::fail(HS_ERR_STATE, "the image holds no cvImgL: its frame came from hs_image_set_raw");
  HS_HIP(hipSetDevice(im->device));
  const size_t n = (size_t)(im->W >> lvl) * (im->H >> lvl);
  std::vector<float4> tex(dirpyr_out ? n : 0);
  hipStream_t s = im->stream;
  if (dirpyr_out) HS_HIP(hipMemcpyAsync(tex.data(), im->d_lvl[lvl], n * sizeof(float4), hipMemcpyDeviceToHost, s));
  if (absg_out) HS_HIP(hipMemcpyAsync(absg_out, im->d_absg[lvl], n * sizeof(float), hipMemcpyDeviceToHost, s));
  if (img8_out) HS_HIP(hipMemcpyAsync(img8_out, im->d_img8, n, hipMemcpyDeviceToHost, s));
  HS_HIP(hipStreamSynchronize(s));
  for (size_t i = 0; i < tex.size(); i++) {
    dirpyr_out[3 * i] = tex[i].x;
    dirpyr_out[3 * i + 1] = tex[i].y;
    dirpyr_out[3 * i + 2] = tex[i].z;
  }
  return HS_OK;
}

int hs_image_last_stats(hs_image* im, double* ms) {
  if (!im) return hs::fail(HS_ERR_INVALID, "null image");
  float f = 0;
  if (im->have) {
    HS_HIP(hipSetDevice(im->device));
    HS_HIP(hipEventSynchronize(im->e1));
    HS_HIP(hipEventElapsedTime(&f, im->e0, im->e1));
  }
  if (ms) *ms = f;
  return HS_OK;
}

}  // extern "C"
