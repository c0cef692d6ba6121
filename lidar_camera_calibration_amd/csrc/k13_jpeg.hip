// K13 jpeg -- the device half of include/ilcc_jpeg.h: quantised DCT coefficients (what csrc/jpeg_entropy.cpp leaves of a
// .jpg file) -> pixels in device memory, where K10, K11 and K11c take them.  It stands for the sample pipeline of
// libjpeg's default decoder (jidctint.c "islow", jdsample.c "fancy" upsampling, jdcolor.c), which cv::imread, MATLAB's
// imread and Pillow run: the bytes are theirs.  The arithmetic is the one the header states; tests/jpeg_ref.py restates it.
//
// k13_idct: EIGHT lanes per 8 x 8 block, lane r owning coefficient row r.
//   load       one 16-byte load per lane (8 int16); the 32 blocks of a workgroup are consecutive in memory, so each
//              wavefront reads 1 KiB contiguous.  The lane multiplies its row by its row of the quantisation table.
//   transpose  among the eight lanes, in registers: three butterfly stages (lane ^ 1, ^ 2, ^ 4), four exchanges each.
//              The first two are DPP quad permutes (VALU rate, no LDS pipe), the third a ds_swizzle.  An LDS
//              transpose would move the same 8 dwords per lane through 2 writes + 8 reads per pass plus address
//              arithmetic and padding against bank conflicts, and allocate 16 KiB a workgroup for nothing it keeps.
//   pass 1     the lane that owns a COLUMN runs the eight-point pass with DESCALE by 11 (libjpeg's order: columns first)
//   transpose  back
//   pass 2     the lane that owns a ROW runs the pass with DESCALE by 18, adds 128, clamps and stores its 8 bytes as
//              one 2-dword store (bytes where the address is not 4-byte aligned, and in a block the image clips).
//   A workgroup is 256 threads = 32 blocks side by side in one block row: every image row gets 256 contiguous bytes.
//   One lane per whole block would need no transpose, but a 1920 x 1200 frame would be 563 wavefronts, fewer than the
//   chip has SIMDs (1024), each holding 64 coefficients in registers and storing 8-byte pieces 8 rows apart.
//   No lane leaves before the exchanges: a block past the row's end is computed on zeros and not stored.
// k13_upsample_colour: K11c's map -- 64 x 4 threads over 256 x 4 pixels, four pixels = 12 bytes per lane, one 3-dword
//   store where the address allows.  A lane reads its 4 luma samples as one dword (the planes are padded to whole
//   blocks and 256-byte aligned) and the 4 chroma samples per plane and row its quad touches as bytes at clamped
//   indices: clamping to the real plane IS libjpeg's edge rule (3 s + s = 4 s), so padding samples never enter.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "host_util.h"
#include "ilcc_hip.h"
#include "ilcc_jpeg.h"
#include "jpeg_block8.h"
#include "jpeg_entropy.h"

namespace ilcc {

constexpr int kIdctThreads = 256;                 // 32 blocks of 8 lanes
constexpr int kBlocksPerGroup = kIdctThreads / 8;
constexpr int kColTx = 64, kColTy = 4, kColQuad = 4;   // k13_upsample_colour: K11c's thread-to-pixel map

struct alignas(16) QuantTable {
  uint16_t q[64];
};

struct IdctArgs {
  const int16_t* coef;       // of this component's first block
  uint8_t* dst;
  int64_t dst_stride;
  int32_t blocks_w, blocks_h;
  int32_t clip_w, clip_h;    // nothing is stored at x >= clip_w or y >= clip_h
  QuantTable quant;
};

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

__global__ __launch_bounds__(kIdctThreads) void k13_idct(IdctArgs a) {
  const int lane8 = threadIdx.x & 7;
  const int bx = blockIdx.x * kBlocksPerGroup + (threadIdx.x >> 3);
  const int by = blockIdx.y;
  const bool live = bx < a.blocks_w;
  int32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    const int16_t* row = a.coef + ((int64_t)by * a.blocks_w + bx) * 64 + lane8 * 8;
    const uint4 c = *reinterpret_cast<const uint4*>(row);
    const uint4 q = reinterpret_cast<const uint4*>(a.quant.q)[lane8];
    const uint32_t cw[4] = {c.x, c.y, c.z, c.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = ((int32_t)(cw[k] << 16) >> 16) * (int32_t)(qw[k] & 0xFFFFu);
      v[2 * k + 1] = ((int32_t)cw[k] >> 16) * (int32_t)(qw[k] >> 16);
    }
  }
  transpose8(v, lane8);
  idct_pass<11>(v);
  transpose8(v, lane8);
  idct_pass<18>(v);
  const int y = by * 8 + lane8, x0 = bx * 8;
  if (!live || y >= a.clip_h) return;
  uint32_t px[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) px[k] = clamp255(v[k] + 128);
  const int n = min(8, a.clip_w - x0);
  uint8_t* p = a.dst + (int64_t)y * a.dst_stride + x0;
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

struct ColourArgs {
  const uint8_t *y, *cb, *cr;        // padded planes, 4-byte aligned, strides multiples of 8
  int32_t y_stride, c_stride;
  int32_t width, height;
  int32_t wc, hc;                    // the chroma planes' real size
  uint8_t* dst;
  int64_t dst_stride;
};

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

template <int MODE>
__global__ __launch_bounds__(kColTx* kColTy) void k13_upsample_colour(ColourArgs a) {
  const int x0 = (blockIdx.x * kColTx + threadIdx.x) * kColQuad;
  const int y = blockIdx.y * kColTy + threadIdx.y;
  if (x0 >= a.width || y >= a.height) return;
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

namespace {

int32_t refuse(const std::string& what) {
  set_global_error("ilcc_jpeg_idct_device: " + what);
  return ILCC_BAD_ARGUMENT;
}

// every plane starts on a 256-byte boundary
uint64_t plane_bytes(const ilcc_jpeg_component& c) { return align256(64ull * (uint64_t)c.blocks_w * (uint64_t)c.blocks_h); }

void launch_idct(const ilcc_jpeg_info& I, int c, const int16_t* d_coef, uint8_t* dst, int64_t stride, int32_t clip_w, int32_t clip_h,
                 hipStream_t s) {
  IdctArgs a;
  a.coef = d_coef + I.comp[c].coef_offset;
  a.dst = dst;
  a.dst_stride = stride;
  a.blocks_w = I.comp[c].blocks_w;
  a.blocks_h = I.comp[c].blocks_h;
  a.clip_w = clip_w;
  a.clip_h = clip_h;
  std::memcpy(a.quant.q, I.quant[I.comp[c].quant_index], sizeof(a.quant.q));
  const dim3 grid((a.blocks_w + kBlocksPerGroup - 1) / kBlocksPerGroup, a.blocks_h);
  hipLaunchKernelGGL(k13_idct, grid, dim3(kIdctThreads), 0, s, a);
}

}  // namespace
}  // namespace ilcc

extern "C" uint64_t ilcc_jpeg_scratch_bytes(const ilcc_jpeg_info* info) {
  using namespace ilcc;
  if (!info || info->n_components != 3 || !jpeg_laid_out(*info)) return 0;
  return plane_bytes(info->comp[0]) + plane_bytes(info->comp[1]) + plane_bytes(info->comp[2]);
}

extern "C" int32_t ilcc_jpeg_idct_device(const ilcc_jpeg_info* info, const int16_t* d_coef, void* d_dst, int32_t dst_stride,
                                         void* d_scratch, uint64_t scratch_bytes, void* hip_stream) {
  using namespace ilcc;
  if (!info || !d_coef || !d_dst) return refuse("null pointer");
  if (!jpeg_laid_out(*info)) return refuse("the info's block counts and offsets are not ilcc_jpeg_layout's");
  const ilcc_jpeg_info& I = *info;
  const int bpp = I.n_components == 1 ? 1 : 3;
  if ((int64_t)dst_stride < (int64_t)bpp * I.width) return refuse("dst_stride is shorter than a row");
  if ((uintptr_t)d_coef & 15u) return refuse("d_coef must be 16-byte aligned");
  hipStream_t s = (hipStream_t)hip_stream;
  if (bpp == 1) {
    launch_idct(I, 0, d_coef, (uint8_t*)d_dst, dst_stride, I.width, I.height, s);
  } else {
    if (!d_scratch || ((uintptr_t)d_scratch & 15u)) return refuse("d_scratch must be a 16-byte aligned device pointer");
    if (scratch_bytes < ilcc_jpeg_scratch_bytes(info)) return refuse("scratch_bytes is less than ilcc_jpeg_scratch_bytes");
    uint8_t* plane[3];
    plane[0] = (uint8_t*)d_scratch;
    plane[1] = plane[0] + plane_bytes(I.comp[0]);
    plane[2] = plane[1] + plane_bytes(I.comp[1]);
    for (int c = 0; c < 3; ++c)   // whole padded planes: nothing clipped
      launch_idct(I, c, d_coef, plane[c], 8 * I.comp[c].blocks_w, 8 * I.comp[c].blocks_w, 8 * I.comp[c].blocks_h, s);
    ColourArgs a;
    a.y = plane[0];
    a.cb = plane[1];
    a.cr = plane[2];
    a.y_stride = 8 * I.comp[0].blocks_w;
    a.c_stride = 8 * I.comp[1].blocks_w;
    a.width = I.width;
    a.height = I.height;
    a.wc = (I.width + I.comp[0].h - 1) / I.comp[0].h;
    a.hc = (I.height + I.comp[0].v - 1) / I.comp[0].v;
    a.dst = (uint8_t*)d_dst;
    a.dst_stride = dst_stride;
    const dim3 block(kColTx, kColTy);
    const dim3 grid((I.width + kColTx * kColQuad - 1) / (kColTx * kColQuad), (I.height + kColTy - 1) / kColTy);
    const bool fancy = a.wc > 2;   // libjpeg takes its "fancy" upsamplers only for planes wider than 2
    if (I.comp[0].h == 1) hipLaunchKernelGGL(k13_upsample_colour<kChroma444>, grid, block, 0, s, a);
    else if (I.comp[0].v == 1 && fancy) hipLaunchKernelGGL(k13_upsample_colour<kChroma422>, grid, block, 0, s, a);
    else if (I.comp[0].v == 1) hipLaunchKernelGGL(k13_upsample_colour<kChroma422Replicate>, grid, block, 0, s, a);
    else if (fancy) hipLaunchKernelGGL(k13_upsample_colour<kChroma420>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k13_upsample_colour<kChroma420Replicate>, grid, block, 0, s, a);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_global_error(std::string("k13 launch: ") + hipGetErrorString(e));
    return ILCC_HIP_ERROR;
  }
  return ILCC_OK;
}
