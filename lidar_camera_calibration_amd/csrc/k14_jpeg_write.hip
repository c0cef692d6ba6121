// K14 jpeg write -- the device half of include/ilcc_jpeg_write.h: pixels in device memory (what K11, K11c and K12 leave)
// -> quantised DCT coefficients in the layout csrc/jpeg_entropy_enc.cpp codes and csrc/jpeg_entropy.cpp decodes.  It
// stands for the sample pipeline of libjpeg's default encoder (jccolor.c, the plain downsamplers of jcsample.c with
// their edge expansion, jfdctint.c "islow", the quantiser of jcdctmgr.c, the dummy blocks of jccoefct.c), which
// cv::imwrite and Pillow run: the coefficients are theirs.  The arithmetic is the one the header states, integers only;
// tests/jpeg_write_ref.py restates it.
//
// k14_colour_downsample: K11c's map -- 64 x 4 threads, four adjacent pixels = 12 bytes per lane, one 3-dword load where
//   the quad lies inside the row and the address allows, bytes at clamped columns otherwise.  The grid covers luma's
//   plane padded to whole MCUs, which is exactly the chroma planes' real block grid times the sampling, so every byte
//   of the three planes is written and k14_fdct_quant never meets an unwritten one.  A lane writes its 4 luma samples as
//   one dword and, per chroma plane, 4 samples (4:4:4, a dword) or 2 (a 16-bit store); for 4:2:0 it takes two pixel rows.
//   The padding rules of the header come out of the index clamps: a pixel column past the image is the last column
//   (columns are replicated BEFORE downsampling); a chroma row j past the real plane takes the pixel rows of row hc - 1
//   (DOWNSAMPLED rows are replicated), of which the second is clamped to the image (an odd last row completes its pair).
// k14_fdct_quant: k13_idct's map run backwards -- EIGHT lanes per 8 x 8 block, 32 blocks of one block row per 256-thread
//   workgroup, so the wavefront's loads of one sample row are 64 contiguous bytes per row and its stores 1 KiB contiguous.
//   load       lane r loads sample row r (8 bytes: one 2-dword load from a plane, or from the image where the block lies
//              inside it and the address allows; bytes at clamped columns otherwise) and subtracts 128
//   pass 1     over ROWS, in the lane, no exchange (libjpeg's order: rows first)
//   transpose  among the eight lanes in registers: K13's butterflies (csrc/jpeg_block8.h)
//   pass 2     the lane that owns a COLUMN; then the quantiser on its 8 coefficients: q = (|c| + d / 2) / d as
//              umulhi(|c| + d / 2, ceil(2^32 / d)), exact for every d = 8 .. 2040 and numerator below 2^18 + 2^10
//              (tests/test_jpeg_write_cpu.py proves it); the host passes both per entry, column-major, in the arguments
//   transpose  back, so lane r holds coefficient row r and stores it as ONE 16-byte store
//   No lane leaves before the exchanges: a block past the row's end is computed on zeros and not stored.
//   Dummy blocks (padding of an interleaved scan to whole MCUs; luma only, at most one column and one row) are
//   RECOMPUTED: the block transforms the samples of the block whose DC libjpeg copies -- min(bx, real_w - 1) in a real
//   row, min(bx | (h - 1), real_w - 1) of the last real row below them -- and zeroes its AC.  A fix-up launch would read
//   the DC back after the first had finished: a second launch and a dependency, for at most one block column and one
//   block row that the same launch transforms at full rate anyway.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "host_util.h"
#include "ilcc_hip.h"
#include "ilcc_jpeg_write.h"
#include "jpeg_block8.h"
#include "jpeg_entropy.h"

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

__global__ __launch_bounds__(kFdctThreads) void k14_fdct_quant(FdctArgs a) {
  const int lane8 = threadIdx.x & 7;
  const int bx = blockIdx.x * kBlocksPerGroup + (threadIdx.x >> 3);
  const int by = blockIdx.y;
  const bool live = bx < a.blocks_w;
  const bool dummy = bx >= a.real_w || by >= a.real_h;
  int32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    // the block whose samples this one transforms: itself, or for a dummy block the one whose DC libjpeg copies
    const int sx = min(by >= a.real_h ? (bx | a.h_mask) : bx, a.real_w - 1);
    const int sy = min(by, a.real_h - 1);
    const int y = min(sy * 8 + lane8, a.clamp_h - 1), x0 = sx * 8;
    const uint8_t* row = a.src + (int64_t)y * a.src_stride;
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
  *reinterpret_cast<uint4*>(a.coef + ((int64_t)by * a.blocks_w + bx) * 64 + lane8 * 8) = out;
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

template <int MODE>
__global__ __launch_bounds__(kColTx* kColTy) void k14_colour_downsample(ColourArgs a) {
  const int x0 = (blockIdx.x * kColTx + threadIdx.x) * kColQuad;   // a multiple of 4: x0 / 2 is an even chroma column
  const int j = blockIdx.y * kColTy + threadIdx.y;                 // luma row, for 4:2:0 the chroma row = pair of luma rows
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

namespace {

int32_t refuse(const std::string& what) {
  set_global_error("ilcc_jpeg_fdct_device: " + what);
  return ILCC_BAD_ARGUMENT;
}

// every plane starts on a 256-byte boundary
uint64_t plane_bytes(const ilcc_jpeg_component& c) { return align256(64ull * (uint64_t)c.blocks_w * (uint64_t)c.blocks_h); }

void launch_fdct(const ilcc_jpeg_info& I, int c, const uint8_t* src, int64_t stride, int32_t clamp_w, int32_t clamp_h, int32_t real_w,
                 int32_t real_h, int16_t* d_coef, hipStream_t s) {
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
  const dim3 grid((a.blocks_w + kBlocksPerGroup - 1) / kBlocksPerGroup, a.blocks_h);
  hipLaunchKernelGGL(k14_fdct_quant, grid, dim3(kFdctThreads), 0, s, a);
}

}  // namespace
}  // namespace k14
}  // namespace ilcc

extern "C" uint64_t ilcc_jpeg_fdct_scratch_bytes(const ilcc_jpeg_info* info) {
  using namespace ilcc::k14;
  if (!info || info->n_components != 3 || !ilcc::jpeg_laid_out(*info)) return 0;
  return plane_bytes(info->comp[0]) + plane_bytes(info->comp[1]) + plane_bytes(info->comp[2]);
}

extern "C" int32_t ilcc_jpeg_fdct_device(const ilcc_jpeg_info* info, const void* d_src, int32_t src_stride, int32_t encoding,
                                         int16_t* d_coef, void* d_scratch, uint64_t scratch_bytes, void* hip_stream) {
  using namespace ilcc;
  using namespace ilcc::k14;
  if (!info || !d_src || !d_coef) return refuse("null pointer");
  if (!jpeg_laid_out(*info)) return refuse("the info's block counts and offsets are not ilcc_jpeg_layout's");
  const ilcc_jpeg_info& I = *info;
  for (int c = 0; c < I.n_components; ++c)
    for (int k = 0; k < 64; ++k)
      if (I.quant[I.comp[c].quant_index][k] < 1 || I.quant[I.comp[c].quant_index][k] > 255) return refuse("quantisation entry outside 1 .. 255");
  const int bpp = I.n_components == 1 ? 1 : 3;
  if (encoding != (bpp == 1 ? ILCC_ENCODING_MONO8 : ILCC_ENCODING_BGR8))
    return refuse("the encoding does not fit the components: mono8 for 1, bgr8 for 3");
  if ((int64_t)src_stride < (int64_t)bpp * I.width) return refuse("src_stride is shorter than a row");
  if ((uintptr_t)d_coef & 15u) return refuse("d_coef must be 16-byte aligned");
  hipStream_t s = (hipStream_t)hip_stream;
  const int32_t real_w = (I.width + 7) / 8, real_h = (I.height + 7) / 8;   // luma's blocks that hold samples
  if (bpp == 1) {
    launch_fdct(I, 0, (const uint8_t*)d_src, src_stride, I.width, I.height, real_w, real_h, d_coef, s);
  } else {
    if (!d_scratch || ((uintptr_t)d_scratch & 15u)) return refuse("d_scratch must be a 16-byte aligned device pointer");
    if (scratch_bytes < ilcc_jpeg_fdct_scratch_bytes(info)) return refuse("scratch_bytes is less than ilcc_jpeg_fdct_scratch_bytes");
    uint8_t* plane[3];
    plane[0] = (uint8_t*)d_scratch;
    plane[1] = plane[0] + plane_bytes(I.comp[0]);
    plane[2] = plane[1] + plane_bytes(I.comp[1]);
    ColourArgs a;
    a.src = (const uint8_t*)d_src;
    a.src_stride = src_stride;
    a.width = I.width;
    a.height = I.height;
    a.hc = (I.height + I.comp[0].v - 1) / I.comp[0].v;
    a.y = plane[0];
    a.cb = plane[1];
    a.cr = plane[2];
    a.y_stride = 8 * I.comp[0].blocks_w;
    a.c_stride = 8 * I.comp[1].blocks_w;
    a.plane_w = 8 * I.comp[0].blocks_w;
    a.plane_h = 8 * I.comp[0].blocks_h;
    const int rows = I.comp[0].v == 2 ? a.plane_h / 2 : a.plane_h;
    const dim3 block(kColTx, kColTy);
    const dim3 grid((a.plane_w + kColTx * kColQuad - 1) / (kColTx * kColQuad), (rows + kColTy - 1) / kColTy);
    if (I.comp[0].h == 1) hipLaunchKernelGGL(k14_colour_downsample<k444>, grid, block, 0, s, a);
    else if (I.comp[0].v == 1) hipLaunchKernelGGL(k14_colour_downsample<k422>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k14_colour_downsample<k420>, grid, block, 0, s, a);
    // chroma's blocks all hold samples; whole planes: nothing clamped
    launch_fdct(I, 0, plane[0], a.y_stride, a.plane_w, a.plane_h, real_w, real_h, d_coef, s);
    for (int c = 1; c < 3; ++c)
      launch_fdct(I, c, plane[c], a.c_stride, a.c_stride, 8 * I.comp[c].blocks_h, I.comp[c].blocks_w, I.comp[c].blocks_h, d_coef, s);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_global_error(std::string("k14 launch: ") + hipGetErrorString(e));
    return ILCC_HIP_ERROR;
  }
  return ILCC_OK;
}
