// hs_undist_tables.cpp — the host tables of include/hs_undist.h: GeometricUndistorter's remap table and K
// (Src/GeometricUndistorter.cpp:20-197 monocular path, makeOptimalK_crop 199-308, distortCoordinates 310-456) and
// PhotometricUndistorter's Binv / B / vignette tables (Src/PhotometricDistorter/photometricUndistorter.cpp:52-108,
// 175-200).  Plain C++17 with no HIP include: g++ alone compiles this file.
//
// The arithmetic is restated operation by operation, with the reference's types: ic[] and K are double there and
// are narrowed to float where distortCoordinates reads them; a double literal in a float expression (2.0 * r1 * mxy,
// minX *= 1.01, ix = 0.001) makes that subexpression double.  The validity pass keeps the reference's quirks.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/hs_ba.h"
#include "../../include/hs_undist.h"
#define HS_HOST_ERRORS_ONLY
#include "hs_host.h"
#include "hs_undist_tables.h"

namespace {
struct Cam {
  int model;
  double ic[8];  // input fx fy cx cy, then the distortion parameters
  double K[4];   // output fx fy cx cy (the reference's Mat33 K, double)
};

// distortCoordinates: output-image coordinates to input-image coordinates, in place
void distort(const Cam& c, float* xs, float* ys, int n) {
  const float fx = (float)c.ic[0], fy = (float)c.ic[1], cx = (float)c.ic[2], cy = (float)c.ic[3];
  const float ofx = (float)c.K[0], ofy = (float)c.K[1], ocx = (float)c.K[2], ocy = (float)c.K[3];
  switch (c.model) {
    case HS_CAM_PINHOLE:
      for (int i = 0; i < n; i++) {
        float ix = (xs[i] - ocx) / ofx;
        float iy = (ys[i] - ocy) / ofy;
        xs[i] = fx * ix + cx;
        ys[i] = fy * iy + cy;
      }
      break;
    case HS_CAM_ATAN: {
      const float dist = (float)c.ic[4];
      const float d2t = 2.0f * std::tan(dist / 2.0f);
      for (int i = 0; i < n; i++) {
        float ix = (xs[i] - ocx) / ofx;
        float iy = (ys[i] - ocy) / ofy;
        const float r = std::sqrt(ix * ix + iy * iy);
        const float fac = (r == 0 || dist == 0) ? 1.0f : std::atan(r * d2t) / (dist * r);
        xs[i] = fx * fac * ix + cx;
        ys[i] = fy * fac * iy + cy;
      }
      break;
    }
    case HS_CAM_RADTAN: {
      const float k1 = (float)c.ic[4], k2 = (float)c.ic[5], r1 = (float)c.ic[6], r2 = (float)c.ic[7];
      for (int i = 0; i < n; i++) {
        const float ix = (xs[i] - ocx) / ofx;
        const float iy = (ys[i] - ocy) / ofy;
        const float mx2 = ix * ix, my2 = iy * iy, mxy = ix * iy;
        const float rho2 = mx2 + my2;
        const float rad = k1 * rho2 + k2 * rho2 * rho2;
        // the tangential terms are double (2.0 is a double literal); the sum is narrowed once
        const float xd = (float)((double)(ix + ix * rad) + 2.0 * (double)r1 * (double)mxy +
                                 (double)r2 * ((double)rho2 + 2.0 * (double)mx2));
        const float yd = (float)((double)(iy + iy * rad) + 2.0 * (double)r2 * (double)mxy +
                                 (double)r1 * ((double)rho2 + 2.0 * (double)my2));
        xs[i] = fx * xd + cx;
        ys[i] = fy * yd + cy;
      }
      break;
    }
    case HS_CAM_EQUIDISTANT: {
      const float k1 = (float)c.ic[4], k2 = (float)c.ic[5], k3 = (float)c.ic[6], k4 = (float)c.ic[7];
      for (int i = 0; i < n; i++) {
        const float ix = (xs[i] - ocx) / ofx;
        const float iy = (ys[i] - ocy) / ofy;
        const float r = std::sqrt(ix * ix + iy * iy);
        const float th = std::atan(r);
        const float th2 = th * th, th4 = th2 * th2, th6 = th4 * th2, th8 = th4 * th4;
        const float thd = th * (1.0f + k1 * th2 + k2 * th4 + k3 * th6 + k4 * th8);
        const float scaling = ((double)r > 1e-8) ? thd / r : 1.0f;
        xs[i] = fx * ix * scaling + cx;
        ys[i] = fy * iy * scaling + cy;
      }
      break;
    }
    default: {  // HS_CAM_KANNALABRANDT
      const float k0 = (float)c.ic[4], k1 = (float)c.ic[5], k2 = (float)c.ic[6], k3 = (float)c.ic[7];
      for (int i = 0; i < n; i++) {
        const float ix = (xs[i] - ocx) / ofx;
        const float iy = (ys[i] - ocy) / ofy;
        const float s = std::sqrt(ix * ix + iy * iy);
        const float th = std::atan2(s, 1.0f);
        const float th2 = th * th, th3 = th2 * th, th5 = th3 * th2, th7 = th5 * th2, th9 = th7 * th2;
        const float r = th + k0 * th3 + k1 * th5 + k2 * th7 + k3 * th9;
        if ((double)s < 1e-6) {
          xs[i] = fx * ix + cx;
          ys[i] = fy * iy + cy;
        } else {
          xs[i] = (r / s) * fx * ix + cx;
          ys[i] = (r / s) * fy * iy + cy;
        }
      }
    }
  }
}

// makeOptimalK_crop: the largest output K whose border rows and columns all map inside the input
int optimal_k_crop(Cam& c, int w, int h, int wOrg, int hOrg) {
  c.K[0] = c.K[1] = 1.0;
  c.K[2] = c.K[3] = 0.0;
  const int NS = 100000;
  std::vector<float> tx(NS), ty(NS);
  float minX = 0, maxX = 0, minY = 0, maxY = 0;
  const float wlim = (float)(wOrg - 1), hlim = (float)(hOrg - 1);
  // 1. the centre lines, stretched as far as they stay inside: a coarse first range
  for (int i = 0; i < NS; i++) {
    tx[i] = ((float)i - 50000.0f) / 10000.0f;
    ty[i] = 0;
  }
  distort(c, tx.data(), ty.data(), NS);
  for (int i = 0; i < NS; i++)
    if (tx[i] > 0 && tx[i] < wlim) {
      if (minX == 0) minX = ((float)i - 50000.0f) / 10000.0f;
      maxX = ((float)i - 50000.0f) / 10000.0f;
    }
  for (int i = 0; i < NS; i++) {
    ty[i] = ((float)i - 50000.0f) / 10000.0f;
    tx[i] = 0;
  }
  distort(c, tx.data(), ty.data(), NS);
  for (int i = 0; i < NS; i++)
    if (ty[i] > 0 && ty[i] < hlim) {
      if (minY == 0) minY = ((float)i - 50000.0f) / 10000.0f;
      maxY = ((float)i - 50000.0f) / 10000.0f;
    }
  minX = (float)((double)minX * 1.01);
  maxX = (float)((double)maxX * 1.01);
  minY = (float)((double)minY * 1.01);
  maxY = (float)((double)maxY * 1.01);

  // 2. while a border has pixels from outside, shrink that side (of two candidates, the wider dimension)
  std::vector<float> bx(2 * (size_t)(w > h ? w : h)), by(bx.size());
  bool oobL = true, oobR = true, oobT = true, oobB = true;
  int iteration = 0;
  while (oobL || oobR || oobT || oobB) {
    oobL = oobR = oobT = oobB = false;
    for (int y = 0; y < h; y++) {
      bx[2 * y] = minX;
      bx[2 * y + 1] = maxX;
      by[2 * y] = by[2 * y + 1] = minY + (maxY - minY) * (float)y / ((float)h - 1.0f);
    }
    distort(c, bx.data(), by.data(), 2 * h);
    for (int y = 0; y < h; y++) {
      if (!(bx[2 * y] > 0 && bx[2 * y] < wlim)) oobL = true;
      if (!(bx[2 * y + 1] > 0 && bx[2 * y + 1] < wlim)) oobR = true;
    }
    for (int x = 0; x < w; x++) {
      by[2 * x] = minY;
      by[2 * x + 1] = maxY;
      bx[2 * x] = bx[2 * x + 1] = minX + (maxX - minX) * (float)x / ((float)w - 1.0f);
    }
    distort(c, bx.data(), by.data(), 2 * w);
    for (int x = 0; x < w; x++) {
      if (!(by[2 * x] > 0 && by[2 * x] < hlim)) oobT = true;
      if (!(by[2 * x + 1] > 0 && by[2 * x + 1] < hlim)) oobB = true;
    }
    if ((oobL || oobR) && (oobT || oobB)) {
      if ((maxX - minX) > (maxY - minY))
        oobB = oobT = false;
      else
        oobL = oobR = false;
    }
    if (oobL) minX = (float)((double)minX * 0.995);
    if (oobR) maxX = (float)((double)maxX * 0.995);
    if (oobT) minY = (float)((double)minY * 0.995);
    if (oobB) maxY = (float)((double)maxY * 0.995);
    iteration++;
    if (iteration > 500) return hs::fail(HS_ERR_INVALID, "crop: no output K found in 500 iterations");
  }
  c.K[0] = (double)(((float)w - 1.0f) / (maxX - minX));
  c.K[1] = (double)(((float)h - 1.0f) / (maxY - minY));
  c.K[2] = (double)(-minX) * c.K[0];
  c.K[3] = (double)(-minY) * c.K[1];
  return HS_OK;
}
}  // namespace

int hs_undist_check_map(const float* remap_x, const float* remap_y, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const float x = remap_x[i], y = remap_y[i];
    if (!(x >= -32767.f && x <= 32767.f && y >= -32767.f && y <= 32767.f))
      return hs::fail(HS_ERR_INVALID, "remap value not finite or outside +-32767");
  }
  return HS_OK;
}

extern "C" int hs_undist_make_remap(const hs_undist_calib* cal, float K_out[4], float* remap_x, float* remap_y) {
  if (!cal || !K_out || !remap_x || !remap_y) return hs::fail(HS_ERR_INVALID, "null argument");
  if (cal->model < HS_CAM_PINHOLE || cal->model > HS_CAM_KANNALABRANDT)
    return hs::fail(HS_ERR_INVALID, "bad camera model");
  if (cal->process < HS_UNDIST_CROP || cal->process > HS_UNDIST_USEK) return hs::fail(HS_ERR_INVALID, "bad process");
  const int w = cal->w_out, h = cal->h_out, wOrg = cal->w_in, hOrg = cal->h_in;
  if (w <= 0 || h <= 0 || wOrg <= 0 || hOrg <= 0 || (long long)w * h >= (1LL << 30) ||
      (long long)wOrg * hOrg >= (1LL << 30))
    return hs::fail(HS_ERR_INVALID, "bad image size");
  if (cal->process == HS_UNDIST_CROP && (w < 2 || h < 2)) return hs::fail(HS_ERR_INVALID, "crop needs an output of 2x2 or more");
  if (cal->process == HS_UNDIST_NONE && (w != wOrg || h != hOrg))
    return hs::fail(HS_ERR_INVALID, "process none requires equal input and output sizes");

  Cam c;
  c.model = cal->model;
  double Kl[4] = {cal->K_in[0], cal->K_in[1], cal->K_in[2], cal->K_in[3]};
  if (Kl[2] < 1 && Kl[3] < 1) {  // relative to the input size
    Kl[0] *= wOrg;
    Kl[1] *= hOrg;
    Kl[2] = Kl[2] * wOrg - 0.5;
    Kl[3] = Kl[3] * hOrg - 0.5;
  }
  for (int i = 0; i < 4; i++) c.ic[i] = Kl[i];
  for (int i = 0; i < 4; i++) c.ic[4 + i] = 0.0;
  if (cal->model == HS_CAM_ATAN)
    c.ic[4] = cal->dist[0];
  else if (cal->model != HS_CAM_PINHOLE)
    for (int i = 0; i < 4; i++) c.ic[4 + i] = cal->dist[i];

  if (cal->process == HS_UNDIST_CROP) {
    int rc = optimal_k_crop(c, w, h, wOrg, hOrg);
    if (rc) return rc;
  } else if (cal->process == HS_UNDIST_NONE) {
    for (int i = 0; i < 4; i++) c.K[i] = Kl[i];
  } else {
    if (cal->desired_K[2] > 1 || cal->desired_K[3] > 1)
      return hs::fail(HS_ERR_INVALID, "desired_K must be relative to the output width and height");
    c.K[0] = cal->desired_K[0] * w;
    c.K[1] = cal->desired_K[1] * h;
    c.K[2] = cal->desired_K[2] * w - 0.5;
    c.K[3] = cal->desired_K[3] * h - 0.5;
  }

  const size_t n = (size_t)w * h;
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      remap_x[x + (size_t)y * w] = (float)x;
      remap_y[x + (size_t)y * w] = (float)y;
    }
  for (int y = 0; y < h; y++) distort(c, remap_x + (size_t)y * w, remap_y + (size_t)y * w, w);

  // the reference's "rounding resistant" pass as written: the second nudge assigns ix from hOrg, and iy is tested
  // against wOrg
  const float wlim = (float)(wOrg - 1), hlim = (float)(hOrg - 1);
  for (size_t i = 0; i < n; i++) {
    float ix = remap_x[i], iy = remap_y[i];
    if (ix == 0) ix = (float)0.001;
    if (iy == 0) iy = (float)0.001;
    if (ix == wlim) ix = (float)(wOrg - 1.001);
    if (iy == hlim) ix = (float)(hOrg - 1.001);
    if (ix > 0 && iy > 0 && ix < wlim && iy < wlim) {
      remap_x[i] = ix;
      remap_y[i] = iy;
    } else {
      remap_x[i] = -1;
      remap_y[i] = -1;
    }
  }
  int rc = hs_undist_check_map(remap_x, remap_y, n);
  if (rc) return rc;
  for (int i = 0; i < 4; i++) K_out[i] = (float)c.K[i];
  return HS_OK;
}

extern "C" int hs_undist_make_photometric(const float* G256, const uint16_t* vignette, int n_in, float Binv[256],
                                          float B[256], float* vignette_inv) {
  if (!Binv || !B) return hs::fail(HS_ERR_INVALID, "null argument");
  if (vignette && (!vignette_inv || n_in <= 0)) return hs::fail(HS_ERR_INVALID, "vignette without an output or a size");
  if (G256) {
    for (int i = 0; i < 256; i++)
      if (!std::isfinite(G256[i])) return hs::fail(HS_ERR_INVALID, "G is not finite");
    for (int i = 0; i < 255; i++)
      if (G256[i + 1] <= G256[i]) return hs::fail(HS_ERR_INVALID, "G must have 256 strictly increasing entries");
    const float mn = G256[0], mx = G256[255];
    for (int i = 0; i < 256; i++) Binv[i] = (float)(255.0 * (double)(G256[i] - mn) / (double)(mx - mn));
  } else {
    for (int i = 0; i < 256; i++) Binv[i] = (float)i;
  }
  // UpdateGamma: B inverts Binv by the first bracketing segment s >= 1; what no segment brackets stays 0
  for (int i = 0; i < 256; i++) B[i] = 0;
  for (int i = 1; i < 255; i++)
    for (int s = 1; s < 255; s++)
      if (Binv[s] <= (float)i && Binv[s + 1] >= (float)i) {
        B[i] = (float)s + ((float)i - Binv[s]) / (Binv[s + 1] - Binv[s]);
        break;
      }
  B[0] = 0;
  B[255] = 255;
  if (vignette) {
    float maxV = 0;
    for (int i = 0; i < n_in; i++)
      if ((float)vignette[i] > maxV) maxV = (float)vignette[i];
    for (int i = 0; i < n_in; i++) vignette_inv[i] = maxV / (float)vignette[i];
  }
  return HS_OK;
}
