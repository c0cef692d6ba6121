// The stages of K13 as __device__ bodies, ONE implementation each, called by the single-image kernels (k13_jpeg.hip) and by
// the batch kernels (k13b_jpeg_batch.hip).  Both files are compiled with the same flags, and the arithmetic is int32
// throughout, so a stage gives the same bytes whichever kernel calls it.  What a kernel adds is only where its block, its
// quantisation row and its planes lie.  Also here: the thread-to-data maps both kernels launch with, and the padded plane
// sizes both hosts lay their scratch out with.  Internal, not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "host_util.h"
#include "ilcc_jpeg.h"
#include "jpeg_block8.h"

namespace ilcc {

constexpr int kIdctThreads = 256;                 // 32 blocks of 8 lanes
constexpr int kBlocksPerGroup = kIdctThreads / 8;
constexpr int kColTx = 64, kColTy = 4, kColQuad = 4;   // upsample_colour: K11c's thread-to-pixel map

// every plane starts on a 256-byte boundary
inline uint64_t jpeg_plane_bytes(const ilcc_jpeg_component& c) { return align256(64ull * (uint64_t)c.blocks_w * (uint64_t)c.blocks_h); }

// libjpeg's jpeg_idct_islow pass (CONST_BITS 13), in place; the caller's SHIFT is 11 (pass 1) or 18 (pass 2)
template <int SHIFT>
__device__ __forceinline__ void idct_pass(int32_t (&c)[8]) {
  int32_t z1 = (c[2] + c[6]) * 4433;
  const int32_t t2 = z1 - c[6] * 15137, t3 = z1 + c[2] * 6270;
  const int32_t t0 = (c[0] + c[4]) * 8192, t1 = (c[0] - c[4]) * 8192;
  const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int32_t o0 = c[7], o1 = c[5], o2 = c[3], o3 = c[1];
  z1 = o0 + o3;
  int32_t z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const int32_t z5 = (z3 + z4) * 9633;
  o0 *= 2446;
  o1 *= 16819;
  o2 *= 25172;
  o3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  o0 += z1 + z3;
  o1 += z2 + z4;
  o2 += z2 + z3;
  o3 += z1 + z4;
  constexpr int32_t kHalf = 1 << (SHIFT - 1);
  c[0] = (t10 + o3 + kHalf) >> SHIFT;
  c[7] = (t10 - o3 + kHalf) >> SHIFT;
  c[1] = (t11 + o2 + kHalf) >> SHIFT;
  c[6] = (t11 - o2 + kHalf) >> SHIFT;
  c[2] = (t12 + o1 + kHalf) >> SHIFT;
  c[5] = (t12 - o1 + kHalf) >> SHIFT;
  c[3] = (t13 + o0 + kHalf) >> SHIFT;
  c[4] = (t13 - o0 + kHalf) >> SHIFT;
}

__device__ __forceinline__ uint32_t clamp255(int32_t v) { return (uint32_t)min(max(v, 0), 255); }

// the lane's row of a block, 8 int16 in one 16-byte word, times its row of the quantisation table
__device__ __forceinline__ void idct_dequantise(const uint4& c, const uint4& q, int32_t (&v)[8]) {
  const uint32_t cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[2 * k] = ((int32_t)(cw[k] << 16) >> 16) * (int32_t)(qw[k] & 0xFFFFu);
    v[2 * k + 1] = ((int32_t)cw[k] >> 16) * (int32_t)(qw[k] >> 16);
  }
}

// Block (bx, by) of a plane whose rows are dst_stride apart: v is the lane's dequantised row lane8 (zeros where !live).  All
// eight lanes of a block, live or not, must arrive here together: the transposes exchange among them.  Nothing is stored at
// x >= clip_w or y >= clip_h.
__device__ __forceinline__ void idct_block(int32_t (&v)[8], int lane8, bool live, int bx, int by, uint8_t* dst, int64_t dst_stride, int32_t clip_w,
                                           int32_t clip_h) {
  transpose8(v, lane8);
  idct_pass<11>(v);
  transpose8(v, lane8);
  idct_pass<18>(v);
  const int y = by * 8 + lane8, x0 = bx * 8;
  if (!live || y >= clip_h) return;
  uint32_t px[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) px[k] = clamp255(v[k] + 128);
  const int n = min(8, clip_w - x0);
  uint8_t* p = dst + (int64_t)y * dst_stride + x0;
  if (n == 8 && ((uintptr_t)p & 3u) == 0) {
    Dword2 d;
    d.x = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    d.y = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
    *reinterpret_cast<Dword2*>(p) = d;
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < n) p[k] = (uint8_t)px[k];
  }
}

enum ChromaMode { kChroma444 = 0, kChroma422 = 1, kChroma420 = 2, kChroma422Replicate = 3, kChroma420Replicate = 4 };

// libjpeg takes its "fancy" upsamplers only for planes wider than 2
inline ChromaMode chroma_mode(const ilcc_jpeg_info& I) {
  const bool fancy = (I.width + I.comp[0].h - 1) / I.comp[0].h > 2;
  if (I.comp[0].h == 1) return kChroma444;
  if (I.comp[0].v == 1) return fancy ? kChroma422 : kChroma422Replicate;
  return fancy ? kChroma420 : kChroma420Replicate;
}

struct ColourArgs {
  const uint8_t *y, *cb, *cr;        // padded planes, 4-byte aligned, strides multiples of 8
  int32_t y_stride, c_stride;
  int32_t width, height;
  int32_t wc, hc;                    // the chroma planes' real size
  uint8_t* dst;
  int64_t dst_stride;
};

// everything of ColourArgs but the pointers, which the caller sets
inline ColourArgs colour_geometry(const ilcc_jpeg_info& I, int64_t dst_stride) {
  ColourArgs a{};
  a.y_stride = 8 * I.comp[0].blocks_w;
  a.c_stride = 8 * I.comp[1].blocks_w;
  a.width = I.width;
  a.height = I.height;
  a.wc = (I.width + I.comp[0].h - 1) / I.comp[0].h;
  a.hc = (I.height + I.comp[0].v - 1) / I.comp[0].v;
  a.dst_stride = dst_stride;
  return a;
}

// the four upsampled chroma samples of pixels x0 .. x0 + 3 in row y (x0 a multiple of 4), from one plane
template <int MODE>
__device__ __forceinline__ void chroma_quad(const uint8_t* plane, const ColourArgs& a, int x0, int y, int32_t (&out)[4]) {
  if constexpr (MODE == kChroma444) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(plane + (int64_t)y * a.c_stride + x0);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = (int32_t)((w >> (8 * k)) & 255u);
  } else if constexpr (MODE == kChroma422Replicate || MODE == kChroma420Replicate) {
    const uint8_t* row = plane + (int64_t)(MODE == kChroma420Replicate ? y >> 1 : y) * a.c_stride;
    const int i0 = x0 >> 1;
    out[0] = out[1] = row[i0];
    out[2] = out[3] = row[min(i0 + 1, a.wc - 1)];
  } else {
    const int i0 = x0 >> 1;
    const int col[4] = {max(i0 - 1, 0), i0, min(i0 + 1, a.wc - 1), min(i0 + 2, a.wc - 1)};
    int32_t r[4];
    if constexpr (MODE == kChroma422) {
      const uint8_t* row = plane + (int64_t)y * a.c_stride;
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = row[col[k]];
      out[0] = (3 * r[1] + r[0] + 1) >> 2;
      out[1] = (3 * r[1] + r[2] + 2) >> 2;
      out[2] = (3 * r[2] + r[1] + 1) >> 2;
      out[3] = (3 * r[2] + r[3] + 2) >> 2;
    } else {
      const int j = y >> 1;
      const int jn = (y & 1) ? min(j + 1, a.hc - 1) : max(j - 1, 0);
      const uint8_t* near_row = plane + (int64_t)j * a.c_stride;
      const uint8_t* far_row = plane + (int64_t)jn * a.c_stride;
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = 3 * (int32_t)near_row[col[k]] + (int32_t)far_row[col[k]];
      out[0] = (3 * r[1] + r[0] + 8) >> 4;
      out[1] = (3 * r[1] + r[2] + 7) >> 4;
      out[2] = (3 * r[2] + r[1] + 8) >> 4;
      out[3] = (3 * r[2] + r[3] + 7) >> 4;
    }
  }
}

// pixels x0 .. x0 + 3 of row y: luma as one dword, chroma upsampled by MODE, B, G, R stored; the caller has checked
// x0 < width and y < height
template <int MODE>
__device__ __forceinline__ void upsample_colour_quad(const ColourArgs& a, int x0, int y) {
  const int n = min(kColQuad, a.width - x0);
  const uint32_t luma = *reinterpret_cast<const uint32_t*>(a.y + (int64_t)y * a.y_stride + x0);
  int32_t cb[4], cr[4];
  chroma_quad<MODE>(a.cb, a, x0, y, cb);
  chroma_quad<MODE>(a.cr, a, x0, y, cr);
  uint32_t px[kColQuad];   // B | G << 8 | R << 16
#pragma unroll
  for (int k = 0; k < kColQuad; ++k) {
    const int32_t Y = (int32_t)((luma >> (8 * k)) & 255u), b = cb[k] - 128, r = cr[k] - 128;
    const uint32_t R = clamp255(Y + ((91881 * r + 32768) >> 16));
    const uint32_t B = clamp255(Y + ((116130 * b + 32768) >> 16));
    const uint32_t G = clamp255(Y + ((-22554 * b - 46802 * r + 32768) >> 16));
    px[k] = B | (G << 8) | (R << 16);
  }
  uint8_t* q = a.dst + (int64_t)y * a.dst_stride + (int64_t)x0 * 3;
  if (n == kColQuad && ((uintptr_t)q & 3u) == 0) {
    Dword3 d;
    d.x = px[0] | (px[1] << 24);
    d.y = (px[1] >> 8) | (px[2] << 16);
    d.z = (px[2] >> 16) | (px[3] << 8);
    *reinterpret_cast<Dword3*>(q) = d;
  } else {
#pragma unroll
    for (int k = 0; k < kColQuad; ++k)
      if (k < n) {
        q[3 * k] = (uint8_t)px[k];
        q[3 * k + 1] = (uint8_t)(px[k] >> 8);
        q[3 * k + 2] = (uint8_t)(px[k] >> 16);
      }
  }
}

}  // namespace ilcc
