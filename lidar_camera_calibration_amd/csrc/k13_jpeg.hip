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
// The stage bodies live in csrc/k13_stages.h, which the batch kernels (K13b, csrc/k13b_jpeg_batch.hip) call too: the
// kernels here only say where a block, its quantisation row and the planes lie.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "host_util.h"
#include "ilcc_hip.h"
#include "ilcc_jpeg.h"
#include "jpeg_block8.h"
#include "jpeg_entropy.h"
#include "k13_stages.h"

namespace ilcc {

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

__global__ __launch_bounds__(kIdctThreads) void k13_idct(IdctArgs a) {
  const int lane8 = threadIdx.x & 7;
  const int bx = blockIdx.x * kBlocksPerGroup + (threadIdx.x >> 3);
  const int by = blockIdx.y;
  const bool live = bx < a.blocks_w;
  int32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    const int16_t* row = a.coef + ((int64_t)by * a.blocks_w + bx) * 64 + lane8 * 8;
    idct_dequantise(*reinterpret_cast<const uint4*>(row), reinterpret_cast<const uint4*>(a.quant.q)[lane8], v);
  }
  idct_block(v, lane8, live, bx, by, a.dst, a.dst_stride, a.clip_w, a.clip_h);
}

template <int MODE>
__global__ __launch_bounds__(kColTx* kColTy) void k13_upsample_colour(ColourArgs a) {
  const int x0 = (blockIdx.x * kColTx + threadIdx.x) * kColQuad;
  const int y = blockIdx.y * kColTy + threadIdx.y;
  if (x0 >= a.width || y >= a.height) return;
  upsample_colour_quad<MODE>(a, x0, y);
}

namespace {

int32_t refuse(const std::string& what) {
  set_global_error("ilcc_jpeg_idct_device: " + what);
  return ILCC_BAD_ARGUMENT;
}

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
  return jpeg_plane_bytes(info->comp[0]) + jpeg_plane_bytes(info->comp[1]) + jpeg_plane_bytes(info->comp[2]);
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
    plane[1] = plane[0] + jpeg_plane_bytes(I.comp[0]);
    plane[2] = plane[1] + jpeg_plane_bytes(I.comp[1]);
    for (int c = 0; c < 3; ++c)   // whole padded planes: nothing clipped
      launch_idct(I, c, d_coef, plane[c], 8 * I.comp[c].blocks_w, 8 * I.comp[c].blocks_w, 8 * I.comp[c].blocks_h, s);
    ColourArgs a = colour_geometry(I, dst_stride);
    a.y = plane[0];
    a.cb = plane[1];
    a.cr = plane[2];
    a.dst = (uint8_t*)d_dst;
    const dim3 block(kColTx, kColTy);
    const dim3 grid((I.width + kColTx * kColQuad - 1) / (kColTx * kColQuad), (I.height + kColTy - 1) / kColTy);
    switch (chroma_mode(I)) {
      case kChroma444: hipLaunchKernelGGL(k13_upsample_colour<kChroma444>, grid, block, 0, s, a); break;
      case kChroma422: hipLaunchKernelGGL(k13_upsample_colour<kChroma422>, grid, block, 0, s, a); break;
      case kChroma422Replicate: hipLaunchKernelGGL(k13_upsample_colour<kChroma422Replicate>, grid, block, 0, s, a); break;
      case kChroma420: hipLaunchKernelGGL(k13_upsample_colour<kChroma420>, grid, block, 0, s, a); break;
      default: hipLaunchKernelGGL(k13_upsample_colour<kChroma420Replicate>, grid, block, 0, s, a); break;
    }
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_global_error(std::string("k13 launch: ") + hipGetErrorString(e));
    return ILCC_HIP_ERROR;
  }
  return ILCC_OK;
}
