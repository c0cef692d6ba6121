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
// The stage bodies and the argument structs live in csrc/k14_stages.h, which K14b (csrc/k14b_jpeg_write_batch.hip) shares.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "host_util.h"
#include "ilcc_hip.h"
#include "ilcc_jpeg_write.h"
#include "jpeg_entropy.h"
#include "k14_stages.h"

namespace ilcc {

namespace k14 {

__global__ __launch_bounds__(kFdctThreads) void k14_fdct_quant(FdctArgs a) {
  fdct_quant_block(a, a.src, a.coef, blockIdx.x * kBlocksPerGroup + (threadIdx.x >> 3), blockIdx.y, threadIdx.x & 7);
}

template <int MODE>
__global__ __launch_bounds__(kColTx* kColTy) void k14_colour_downsample(ColourArgs a) {
  colour_downsample_quad<MODE>(a, (blockIdx.x * kColTx + threadIdx.x) * kColQuad, blockIdx.y * kColTy + threadIdx.y);
}

namespace {

int32_t refuse(const std::string& what) {
  set_global_error("ilcc_jpeg_fdct_device: " + what);
  return ILCC_BAD_ARGUMENT;
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
  ColourArgs ca{};
  if (bpp == 3) {
    if (!d_scratch || ((uintptr_t)d_scratch & 15u)) return refuse("d_scratch must be a 16-byte aligned device pointer");
    if (scratch_bytes < ilcc_jpeg_fdct_scratch_bytes(info)) return refuse("scratch_bytes is less than ilcc_jpeg_fdct_scratch_bytes");
    ca = colour_args(I, d_src, src_stride, (uint8_t*)d_scratch);
    const int rows = I.comp[0].v == 2 ? ca.plane_h / 2 : ca.plane_h;
    const dim3 block(kColTx, kColTy);
    const dim3 grid((ca.plane_w + kColTx * kColQuad - 1) / (kColTx * kColQuad), (rows + kColTy - 1) / kColTy);
    if (I.comp[0].h == 1) hipLaunchKernelGGL(k14_colour_downsample<k444>, grid, block, 0, s, ca);
    else if (I.comp[0].v == 1) hipLaunchKernelGGL(k14_colour_downsample<k422>, grid, block, 0, s, ca);
    else hipLaunchKernelGGL(k14_colour_downsample<k420>, grid, block, 0, s, ca);
  }
  FdctArgs fa[3];
  fdct_args_all(I, d_src, src_stride, &ca, d_coef, fa);
  for (int c = 0; c < I.n_components; ++c) {
    const dim3 grid((fa[c].blocks_w + kBlocksPerGroup - 1) / kBlocksPerGroup, fa[c].blocks_h);
    hipLaunchKernelGGL(k14_fdct_quant, grid, dim3(kFdctThreads), 0, s, fa[c]);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_global_error(std::string("k14 launch: ") + hipGetErrorString(e));
    return ILCC_HIP_ERROR;
  }
  return ILCC_OK;
}
