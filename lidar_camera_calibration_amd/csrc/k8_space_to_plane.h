// spaceToPlane of ImageCornersEst (src/ImageCornersEst.cpp:135-155), the ONE projection of K8 (k8_project.hip) and K8b
// (k8b_colourise_batch.hip).  Both files are compiled with -ffp-contract=off, so a point takes the same keep decision and the
// same pixel in either; K8b's byte-for-byte contract with ilcc_colourise_device rests on that.
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

}  // namespace ilcc
