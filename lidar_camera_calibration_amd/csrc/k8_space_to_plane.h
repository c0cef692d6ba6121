// spaceToPlane of ImageCornersEst (src/ImageCornersEst.cpp:135-155), the ONE projection of K8 (k8_project.hip), K8b
// (k8b_colourise_batch.hip) and K12b (k12b_overlay_batch.hip), and pcd2image's colour of a point, the one body of K8 and K12b.
// All three files are compiled with -ffp-contract=off, so a point takes the same keep decision, the same pixel and the same
// colour in each; the byte-for-byte contracts of K8b and K12b with K8's entries rest on that.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ilcc_project.h"

namespace ilcc {

constexpr int kProjThreads = 256;
constexpr int kProjChunk = 4096;   // points per workgroup, in both files

// spaceToPlane (:135-155); px, py = the (int) truncation the callers apply
__device__ __forceinline__ bool space_to_plane(const ilcc_projection& c, const float4 q, double dis, int32_t& px, int32_t& py) {
  const double X = (double)q.x, Y = (double)q.y, Z = (double)q.z;
  const double pc0 = c.R[0] * X + c.R[1] * Y + c.R[2] * Z + c.t[0];
  const double pc1 = c.R[3] * X + c.R[4] * Y + c.R[5] * Z + c.t[1];
  const double pc2 = c.R[6] * X + c.R[7] * Y + c.R[8] * Z + c.t[2];
  if (pc2 < 0 || pc2 > dis) return false;   // NaN depth passes this test, like the reference, and fails below
  const double u = pc0 / pc2, v = pc1 / pc2;
  const double cu = c.fx * u + c.cx, cv = c.fy * v + c.cy;
  if (cu > 0 && cu < (double)c.width && cv > 0 && cv < (double)c.height) {
    px = (int32_t)cu;
    py = (int32_t)cv;
    return true;
  }
  return false;
}

// rgblidar.cpp:63-65: the B,G,R pixel at (px, py) as PCL's packed rgb
__device__ __forceinline__ uint32_t sample_bgr_as_rgb(const uint8_t* image, uint32_t image_step, int32_t px, int32_t py) {
  const uint8_t* p = image + (uint64_t)py * image_step + (uint32_t)px * 3u;
  return ((uint32_t)p[2] << 16) | ((uint32_t)p[1] << 8) | (uint32_t)p[0];
}

// ---- pcd2image's colour of a point, the ONE body of K8 (ilcc_project_intensity_device) and K12b (k12b_overlay_batch.hip) ----

// float -> unsigned char the way an x86-64 build converts (cvttss2si, low byte)
__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)(int32_t)v; }
// double -> int as cvttsd2si: NaN / out of range give INT_MIN ("integer indefinite"), not saturation
__device__ __forceinline__ int32_t x86_d2i(double v) {
  return (v > -2147483649.0 && v < 2147483648.0) ? (int32_t)v : (int32_t)0x80000000;
}

// HSVtoRGB (:373-428) with s = v = 100
__device__ __forceinline__ void hsv_to_rgb(int32_t h, int32_t s, int32_t v, uint8_t& r, uint8_t& g, uint8_t& b) {
  const float rgb_max = v * 2.55f;
  const float rgb_min = rgb_max * (100 - s) / 100.0f;
  const int32_t i = h / 60;
  const int32_t difs = h % 60;
  const float adj = (rgb_max - rgb_min) * difs / 60.0f;
  switch (i) {
    case 0: r = to_u8(rgb_max); g = to_u8(rgb_min + adj); b = to_u8(rgb_min); break;
    case 1: r = to_u8(rgb_max - adj); g = to_u8(rgb_max); b = to_u8(rgb_min); break;
    case 2: r = to_u8(rgb_min); g = to_u8(rgb_max); b = to_u8(rgb_min + adj); break;
    case 3: r = to_u8(rgb_min); g = to_u8(rgb_max - adj); b = to_u8(rgb_max); break;
    case 4: r = to_u8(rgb_min + adj); g = to_u8(rgb_min); b = to_u8(rgb_max); break;
    default: r = to_u8(rgb_max); g = to_u8(rgb_min); b = to_u8(rgb_max - adj); break;
  }
}

// pcd2image.cpp:71-73: the hue of an intensity in lo .. hi, then HSVtoRGB(hue, 100, 100); r | g << 8 | b << 16 as ilcc_pixel_hit holds it
__device__ __forceinline__ uint32_t intensity_rgb(float intensity, double lo, double hi) {
  const double h = ((double)intensity - lo) / (hi - lo) * 255;   // pcd2image.cpp:71
  uint8_t r, g, b;
  hsv_to_rgb(x86_d2i(h), 100, 100, r, g, b);
  return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}

}  // namespace ilcc
