// What K0 (one message per launch) and K0b (a batch of messages per launch) share: the arguments of one message, the rule that
// picks its path, and the device code for a tile and for a generic point.  Internal, not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ilcc_ingest.h"

namespace ilcc {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kUnpackThreads = 256;
constexpr int kUnpackTile = 1024;   // points per workgroup of the tiled path (the generic path: kUnpackThreads)

struct UnpackArgs {
  const uint8_t* src;
  float4* dst;
  uint64_t n_points;
  uint32_t width, point_step, row_step;
  uint32_t off[4];   // x y z intensity, ILCC_FIELD_ABSENT -> 0
};

inline void unpack_args_from_layout(const ilcc_pointcloud2_layout& L, const void* d_data, void* d_xyzi, UnpackArgs* a) {
  a->src = (const uint8_t*)d_data;
  a->dst = (float4*)d_xyzi;
  a->n_points = (uint64_t)L.height * L.width;
  a->width = L.width;
  a->point_step = L.point_step;
  a->row_step = L.row_step;
  a->off[0] = L.off_x;
  a->off[1] = L.off_y;
  a->off[2] = L.off_z;
  a->off[3] = L.off_intensity;
}

// The path of a message whose data[] starts at d_data: 1..4 = tiled with point_step 16..64 (point_step % 16 == 0, field offsets
// % 4 == 0, source 16-byte aligned, rows packed), 0 = generic
inline int unpack_class(const ilcc_pointcloud2_layout& L, const void* d_data) {
  bool aligned = (L.point_step % 16 == 0) && L.point_step <= 64 && ((uintptr_t)d_data % 16 == 0) &&
                 (L.height == 1 || L.row_step == (uint64_t)L.width * L.point_step);
  for (uint32_t off : {L.off_x, L.off_y, L.off_z, L.off_intensity}) aligned = aligned && (off == ILCC_FIELD_ABSENT || off % 4 == 0);
  return aligned ? (int)(L.point_step / 16) : 0;
}

#ifdef __HIPCC__
__device__ __forceinline__ float load_f32_bytes(const uint8_t* p) {
  const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
  return __uint_as_float(v);
}

// point i of the message, any alignment, any padding
__device__ __forceinline__ void unpack_generic_point(const UnpackArgs& a, uint64_t i) {
  if (i >= a.n_points) return;
  const uint64_t row = i / a.width, col = i - row * a.width;
  const uint8_t* p = a.src + row * a.row_step + col * a.point_step;
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = (a.off[k] == ILCC_FIELD_ABSENT) ? 0.f : load_f32_bytes(p + a.off[k]);
  a.dst[i] = make_float4(v[0], v[1], v[2], v[3]);
}

// points [p0, p0 + kUnpackTile) of the message by one workgroup of kUnpackThreads, staged through `tile` (kUnpackTile * STEP16
// pieces of LDS).  STEP16 = point_step / 16 (1..4): points are packed back to back (row_step == width * point_step)
template <int STEP16>
__device__ __forceinline__ void unpack_tile(const UnpackArgs& a, uint64_t p0, u32x4* tile) {
  const uint64_t left = a.n_points - p0;
  const uint32_t pts = left < (uint64_t)kUnpackTile ? (uint32_t)left : (uint32_t)kUnpackTile;
  const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(a.src) + p0 * STEP16;
  const uint32_t pieces = pts * STEP16;
#pragma unroll
  for (int k = 0; k < (kUnpackTile * STEP16) / kUnpackThreads; ++k) {
    const uint32_t j = k * kUnpackThreads + threadIdx.x;
    if (j < pieces) tile[j] = __builtin_nontemporal_load(src + j);
  }
  __syncthreads();
  const uint32_t* words = reinterpret_cast<const uint32_t*>(tile);
#pragma unroll
  for (int k = 0; k < kUnpackTile / kUnpackThreads; ++k) {
    const uint32_t j = k * kUnpackThreads + threadIdx.x;
    if (j < pts) {
      const uint32_t* w = words + j * (STEP16 * 4);
      float v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = (a.off[c] == ILCC_FIELD_ABSENT) ? 0.f : __uint_as_float(w[a.off[c] >> 2]);
      a.dst[p0 + j] = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}
#endif

}  // namespace ilcc
