// The stage bodies of K14 (csrc/k14_jpeg_write.hip), shared with K14b (csrc/k14b_jpeg_write_batch.hip), which runs them on a
// batch with the image as a grid dimension: the thread-to-data maps, the arithmetic and the argument structs are stated once,
// here, and both files compile them with the same flags, so a batch's coefficients are K14's byte for byte.  What the stages
// do and why is told at the top of csrc/k14_jpeg_write.hip.
#ifndef ILCC_K14_STAGES_H_
#define ILCC_K14_STAGES_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "host_util.h"
#include "ilcc_jpeg.h"
#include "jpeg_block8.h"

namespace ilcc {
namespace k14 {

constexpr int kFdctThreads = 256;                 // 32 blocks of 8 lanes
constexpr int kBlocksPerGroup = kFdctThreads / 8;
constexpr int kColTx = 64, kColTy = 4, kColQuad = 4;   // k14_colour_downsample: K11c's thread-to-pixel map

struct FdctArgs {
  const uint8_t* src;        // the image (1 component) or a padded plane
  int64_t src_stride;
  int32_t clamp_w, clamp_h;  // sample indices are clamped to [0, clamp_w) x [0, clamp_h)
  int16_t* coef;             // of this component's first block
  int32_t blocks_w, blocks_h;   // padded to whole MCUs: the grid that is written
  int32_t real_w, real_h;       // blocks that hold samples; the rest are dummy blocks
  int32_t h_mask;               // the component's horizontal sampling factor - 1
  alignas(16) uint32_t recip[64];   // ceil(2^32 / (8 quant)), COLUMN-major: [column * 8 + row]
  alignas(16) uint16_t half[64];    // 4 quant = (8 quant) >> 1, column-major
};

// libjpeg's jpeg_fdct_islow pass (CONST_BITS 13, PASS1_BITS 2), in place
template <bool FIRST>
__device__ __forceinline__ void fdct_pass(int32_t (&d)[8]) {
  constexpr int S = FIRST ? 11 : 15;
  constexpr int32_t kHalf = 1 << (S - 1);
  const int32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int32_t t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if constexpr (FIRST) {
    d[0] = (t10 + t11) * 4;
    d[4] = (t10 - t11) * 4;
  } else {
    d[0] = (t10 + t11 + 2) >> 2;
    d[4] = (t10 - t11 + 2) >> 2;
  }
  int32_t z1 = (t12 + t13) * 4433;
  d[2] = (z1 + t13 * 6270 + kHalf) >> S;
  d[6] = (z1 - t12 * 15137 + kHalf) >> S;
  z1 = t4 + t7;
  int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int32_t z5 = (z3 + z4) * 9633;
  const int32_t p4 = t4 * 2446, p5 = t5 * 16819, p6 = t6 * 25172, p7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7] = (p4 + z1 + z3 + kHalf) >> S;
  d[5] = (p5 + z2 + z4 + kHalf) >> S;
  d[3] = (p6 + z2 + z3 + kHalf) >> S;
  d[1] = (p7 + z1 + z4 + kHalf) >> S;
}

// One lane's share of block (bx, by) of the component `a` describes: load, both passes, the quantiser, the store.  `src` and
// `coef` stand for a.src and a.coef (K14b passes the image's own).  Every lane of a workgroup runs it, live or not: no lane
// leaves before the exchanges.
__device__ __forceinline__ void fdct_quant_block(const FdctArgs& a, const uint8_t* src, int16_t* coef, int bx, int by, int lane8) {
  const bool live = bx < a.blocks_w;
  const bool dummy = bx >= a.real_w || by >= a.real_h;
  int32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    // the block whose samples this one transforms: itself, or for a dummy block the one whose DC libjpeg copies
    const int sx = min(by >= a.real_h ? (bx | a.h_mask) : bx, a.real_w - 1);
    const int sy = min(by, a.real_h - 1);
    const int y = min(sy * 8 + lane8, a.clamp_h - 1), x0 = sx * 8;
    const uint8_t* row = src + (int64_t)y * a.src_stride;
    if (x0 + 8 <= a.clamp_w && ((uintptr_t)(row + x0) & 3u) == 0) {
      const Dword2 w = *reinterpret_cast<const Dword2*>(row + x0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = (int32_t)((w.x >> (8 * k)) & 255u) - 128;
        v[4 + k] = (int32_t)((w.y >> (8 * k)) & 255u) - 128;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = (int32_t)row[min(x0 + k, a.clamp_w - 1)] - 128;
    }
  }
  fdct_pass<true>(v);
  transpose8(v, lane8);
  fdct_pass<false>(v);
  {   // the lane holds column lane8: v[k] is the coefficient of row k
    const uint4 r0 = reinterpret_cast<const uint4*>(a.recip)[2 * lane8], r1 = reinterpret_cast<const uint4*>(a.recip)[2 * lane8 + 1];
    const uint4 h = reinterpret_cast<const uint4*>(a.half)[lane8];
    const uint32_t recip[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    const uint32_t half[8] = {h.x & 0xFFFFu, h.x >> 16, h.y & 0xFFFFu, h.y >> 16, h.z & 0xFFFFu, h.z >> 16, h.w & 0xFFFFu, h.w >> 16};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t mag = (uint32_t)(v[k] < 0 ? -v[k] : v[k]);
      const int32_t q = (int32_t)__umulhi(mag + half[k], recip[k]);
      v[k] = v[k] < 0 ? -q : q;
      if (dummy && (k != 0 || lane8 != 0)) v[k] = 0;
    }
  }
  transpose8(v, lane8);
  if (!live) return;
  uint4 out;
  out.x = ((uint32_t)v[0] & 0xFFFFu) | ((uint32_t)v[1] << 16);
  out.y = ((uint32_t)v[2] & 0xFFFFu) | ((uint32_t)v[3] << 16);
  out.z = ((uint32_t)v[4] & 0xFFFFu) | ((uint32_t)v[5] << 16);
  out.w = ((uint32_t)v[6] & 0xFFFFu) | ((uint32_t)v[7] << 16);
  *reinterpret_cast<uint4*>(coef + ((int64_t)by * a.blocks_w + bx) * 64 + lane8 * 8) = out;
}

enum Sampling { k444 = 0, k422 = 1, k420 = 2 };

struct ColourArgs {
  const uint8_t* src;                // B, G, R
  int64_t src_stride;
  int32_t width, height;
  int32_t hc;                        // the chroma planes' real height: ceil(height / v)
  uint8_t *y, *cb, *cr;              // padded planes, 4-byte aligned, strides multiples of 8
  int32_t y_stride, c_stride;
  int32_t plane_w, plane_h;          // of luma's plane: multiples of 8 (of 16 where chroma is halved)
};

// Y, Cb, Cr of pixels x0 .. x0 + 3 (columns clamped to the image) of pixel row `y` (inside the image)
__device__ __forceinline__ void convert_quad(const ColourArgs& a, int x0, int y, int32_t (&Y)[4], int32_t (&Cb)[4], int32_t (&Cr)[4]) {
  const uint8_t* row = a.src + (int64_t)y * a.src_stride;
  uint32_t px[4];   // B | G << 8 | R << 16
  const uint8_t* p = row + (int64_t)x0 * 3;
  if (x0 + kColQuad <= a.width && ((uintptr_t)p & 3u) == 0) {
    const Dword3 d = *reinterpret_cast<const Dword3*>(p);
    px[0] = d.x & 0xFFFFFFu;
    px[1] = (d.x >> 24) | ((d.y & 0xFFFFu) << 8);
    px[2] = (d.y >> 16) | ((d.z & 0xFFu) << 16);
    px[3] = d.z >> 8;
  } else {
#pragma unroll
    for (int k = 0; k < kColQuad; ++k) {
      const uint8_t* q = row + (int64_t)min(x0 + k, a.width - 1) * 3;
      px[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    }
  }
#pragma unroll
  for (int k = 0; k < kColQuad; ++k) {
    const int32_t B = (int32_t)(px[k] & 255u), G = (int32_t)((px[k] >> 8) & 255u), R = (int32_t)(px[k] >> 16);
    Y[k] = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    Cb[k] = (-11059 * R - 21709 * G + 32768 * B + 8421375) >> 16;
    Cr[k] = (32768 * R - 27439 * G - 5329 * B + 8421375) >> 16;
  }
}

__device__ __forceinline__ uint32_t pack4(const int32_t (&s)[4]) {
  return (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
}

// the lane whose quad starts at luma column x0 (a multiple of 4: x0 / 2 is an even chroma column) of row j: a luma row, for 4:2:0
// the chroma row = pair of luma rows
template <int MODE>
__device__ __forceinline__ void colour_downsample_quad(const ColourArgs& a, int x0, int j) {
  if (x0 >= a.plane_w || j >= (MODE == k420 ? a.plane_h / 2 : a.plane_h)) return;
  int32_t Y[4], Cb[4], Cr[4];
  if constexpr (MODE != k420) {
    convert_quad(a, x0, min(j, a.height - 1), Y, Cb, Cr);
    *reinterpret_cast<uint32_t*>(a.y + (int64_t)j * a.y_stride + x0) = pack4(Y);
    if constexpr (MODE == k444) {
      *reinterpret_cast<uint32_t*>(a.cb + (int64_t)j * a.c_stride + x0) = pack4(Cb);
      *reinterpret_cast<uint32_t*>(a.cr + (int64_t)j * a.c_stride + x0) = pack4(Cr);
    } else {   // bias 0, 1 by output column
      const uint32_t cb = (uint32_t)((Cb[0] + Cb[1]) >> 1) | ((uint32_t)((Cb[2] + Cb[3] + 1) >> 1) << 8);
      const uint32_t cr = (uint32_t)((Cr[0] + Cr[1]) >> 1) | ((uint32_t)((Cr[2] + Cr[3] + 1) >> 1) << 8);
      *reinterpret_cast<uint16_t*>(a.cb + (int64_t)j * a.c_stride + x0 / 2) = (uint16_t)cb;
      *reinterpret_cast<uint16_t*>(a.cr + (int64_t)j * a.c_stride + x0 / 2) = (uint16_t)cr;
    }
  } else {
    // the two pixel rows of chroma row min(j, hc - 1); the second is the image's last row whenever j >= hc - 1 and is
    // then luma's row too for every row below the image
    const int jc = min(j, a.hc - 1);
    const int ra = min(2 * jc, a.height - 1), rb = min(2 * jc + 1, a.height - 1);
    int32_t Y2[4], Cb2[4], Cr2[4];
    convert_quad(a, x0, ra, Y, Cb, Cr);
    convert_quad(a, x0, rb, Y2, Cb2, Cr2);
    const bool below = j >= a.hc;   // both luma rows lie below the image
    *reinterpret_cast<uint32_t*>(a.y + (int64_t)(2 * j) * a.y_stride + x0) = pack4(below ? Y2 : Y);
    *reinterpret_cast<uint32_t*>(a.y + (int64_t)(2 * j + 1) * a.y_stride + x0) = pack4(Y2);
    // bias 1, 2 by output column
    const uint32_t cb = (uint32_t)((Cb[0] + Cb[1] + Cb2[0] + Cb2[1] + 1) >> 2) | ((uint32_t)((Cb[2] + Cb[3] + Cb2[2] + Cb2[3] + 2) >> 2) << 8);
    const uint32_t cr = (uint32_t)((Cr[0] + Cr[1] + Cr2[0] + Cr2[1] + 1) >> 2) | ((uint32_t)((Cr[2] + Cr[3] + Cr2[2] + Cr2[3] + 2) >> 2) << 8);
    *reinterpret_cast<uint16_t*>(a.cb + (int64_t)j * a.c_stride + x0 / 2) = (uint16_t)cb;
    *reinterpret_cast<uint16_t*>(a.cr + (int64_t)j * a.c_stride + x0 / 2) = (uint16_t)cr;
  }
}

// ---- what the two entries share on the host --------------------------------------------------------------------------------

// every plane starts on a 256-byte boundary
inline uint64_t plane_bytes(const ilcc_jpeg_component& c) { return align256(64ull * (uint64_t)c.blocks_w * (uint64_t)c.blocks_h); }

// component c of an image laid out as I: its source (the image, or a padded plane), clamps, real blocks and quantiser
inline FdctArgs fdct_args(const ilcc_jpeg_info& I, int c, const uint8_t* src, int64_t stride, int32_t clamp_w, int32_t clamp_h, int32_t real_w,
                          int32_t real_h, int16_t* d_coef) {
  FdctArgs a;
  a.src = src;
  a.src_stride = stride;
  a.clamp_w = clamp_w;
  a.clamp_h = clamp_h;
  a.coef = d_coef + I.comp[c].coef_offset;
  a.blocks_w = I.comp[c].blocks_w;
  a.blocks_h = I.comp[c].blocks_h;
  a.real_w = real_w;
  a.real_h = real_h;
  a.h_mask = I.comp[c].h - 1;
  const uint16_t* quant = I.quant[I.comp[c].quant_index];
  for (int col = 0; col < 8; ++col)
    for (int row = 0; row < 8; ++row) {
      const uint64_t d = 8ull * quant[row * 8 + col];
      a.recip[col * 8 + row] = (uint32_t)(((1ull << 32) + d - 1) / d);   // ceil(2^32 / d) <= 2^29
      a.half[col * 8 + row] = (uint16_t)(d >> 1);
    }
  return a;
}

// the colour stage of an image laid out as I whose three planes start at `planes`
inline ColourArgs colour_args(const ilcc_jpeg_info& I, const void* d_src, int64_t src_stride, uint8_t* planes) {
  ColourArgs a;
  a.src = (const uint8_t*)d_src;
  a.src_stride = src_stride;
  a.width = I.width;
  a.height = I.height;
  a.hc = (I.height + I.comp[0].v - 1) / I.comp[0].v;
  a.y = planes;
  a.cb = a.y + plane_bytes(I.comp[0]);
  a.cr = a.cb + plane_bytes(I.comp[1]);
  a.y_stride = 8 * I.comp[0].blocks_w;
  a.c_stride = 8 * I.comp[1].blocks_w;
  a.plane_w = 8 * I.comp[0].blocks_w;
  a.plane_h = 8 * I.comp[0].blocks_h;
  return a;
}

// the FdctArgs of the three components of a colour image whose planes `ca` names, or of a gray image read in place
inline void fdct_args_all(const ilcc_jpeg_info& I, const void* d_src, int64_t src_stride, const ColourArgs* ca, int16_t* d_coef, FdctArgs (&out)[3]) {
  const int32_t real_w = (I.width + 7) / 8, real_h = (I.height + 7) / 8;   // luma's blocks that hold samples
  if (I.n_components == 1) {
    out[0] = fdct_args(I, 0, (const uint8_t*)d_src, src_stride, I.width, I.height, real_w, real_h, d_coef);
    return;
  }
  // chroma's blocks all hold samples; whole planes: nothing clamped
  out[0] = fdct_args(I, 0, ca->y, ca->y_stride, ca->plane_w, ca->plane_h, real_w, real_h, d_coef);
  out[1] = fdct_args(I, 1, ca->cb, ca->c_stride, ca->c_stride, 8 * I.comp[1].blocks_h, I.comp[1].blocks_w, I.comp[1].blocks_h, d_coef);
  out[2] = fdct_args(I, 2, ca->cr, ca->c_stride, ca->c_stride, 8 * I.comp[2].blocks_h, I.comp[2].blocks_w, I.comp[2].blocks_h, d_coef);
}

}  // namespace k14
}  // namespace ilcc

#endif
