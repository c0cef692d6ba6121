// K14b -- K14 on a batch of images of one geometry and one set of quantisation tables (include/ilcc_jpeg_write_sequence.h): the
// pixels of n images -> n coefficient arrays, in TWO launches for a colour batch and ONE for a gray batch, whatever n is.  The
// stage bodies are K14's own (csrc/k14_stages.h), compiled with the same flags: every int16 equals what ilcc_jpeg_fdct_device
// writes for that image alone.
//
// k14b_colour_downsample: K14's map (64 x 4 threads, four pixels a lane) with the image as blockIdx.z.  Image m's planes lie at
//   d_scratch + m * ilcc_jpeg_fdct_scratch_bytes(layout), each padded and on a 256-byte boundary as in K14.
// k14b_fdct_quant: one launch for all components of all images, gridded as k13b_idct is.
//   z   the image: base addresses only (pixels or planes, coefficients), scalar arithmetic on blockIdx.z.
//   y   (component, block row) flattened: rows [0, h0) are luma's, [h0, h0 + h1) Cb's, the rest Cr's.  Two wave-uniform compares
//       find the component, whose arguments (the quantiser's reciprocals among them) stay in the kernel-argument segment.
//   x   the 32-block group, sized for luma.  A group that starts past the end of a narrower component's row leaves as a whole,
//       so no lane leaves before the exchanges.
#include <hip/hip_runtime.h>

#include <string>

#include "host_util.h"
#include "ilcc_hip.h"
#include "ilcc_jpeg_write.h"
#include "ilcc_jpeg_write_sequence.h"
#include "jpeg_entropy.h"
#include "k14_stages.h"

namespace ilcc {
namespace k14 {

struct FdctBatchArgs {
  FdctArgs comp[3];          // image 0's
  int32_t first_row[3];      // of the component in the flattened blockIdx.y
  uint64_t src_pitch;        // bytes between the images' pixels (1 component) or planes
  uint64_t coef_pitch;       // int16 between the images' coefficients
};

__global__ __launch_bounds__(kFdctThreads) void k14b_fdct_quant(FdctBatchArgs b) {
  const int row = blockIdx.y;
  const int c = (row >= b.first_row[1] ? 1 : 0) + (row >= b.first_row[2] ? 1 : 0);   // wave-uniform
  const FdctArgs& a = c == 0 ? b.comp[0] : c == 1 ? b.comp[1] : b.comp[2];
  if ((int)(blockIdx.x * kBlocksPerGroup) >= a.blocks_w) return;   // the whole workgroup: this component's rows are narrower
  const uint64_t m = blockIdx.z;
  const int first = c == 0 ? b.first_row[0] : c == 1 ? b.first_row[1] : b.first_row[2];
  fdct_quant_block(a, a.src + m * b.src_pitch, a.coef + m * b.coef_pitch, blockIdx.x * kBlocksPerGroup + (threadIdx.x >> 3), row - first,
                   threadIdx.x & 7);
}

struct ColourBatchArgs {
  ColourArgs image0;         // image 0's pixels and planes
  uint64_t src_pitch;        // bytes between the images' pixels
  uint64_t plane_pitch;      // bytes between the images' planes
};

template <int MODE>
__global__ __launch_bounds__(kColTx* kColTy) void k14b_colour_downsample(ColourBatchArgs b) {
  const uint64_t m = blockIdx.z;
  ColourArgs a = b.image0;
  a.src += m * b.src_pitch;
  a.y += m * b.plane_pitch;
  a.cb += m * b.plane_pitch;
  a.cr += m * b.plane_pitch;
  colour_downsample_quad<MODE>(a, (blockIdx.x * kColTx + threadIdx.x) * kColQuad, blockIdx.y * kColTy + threadIdx.y);
}

namespace {

int32_t refuse_batch(const std::string& what) {
  set_global_error("ilcc_jpeg_fdct_batch_device: " + what);
  return ILCC_BAD_ARGUMENT;
}

}  // namespace
}  // namespace k14
}  // namespace ilcc

extern "C" uint64_t ilcc_jpeg_fdct_batch_scratch_bytes(const ilcc_jpeg_info* layout, uint32_t n_images) {
  return ilcc_jpeg_fdct_scratch_bytes(layout) * (uint64_t)n_images;
}

extern "C" int32_t ilcc_jpeg_fdct_batch_device(const ilcc_jpeg_fdct_batch_job* job) {
  using namespace ilcc;
  using namespace ilcc::k14;
  if (!job || !job->layout || !job->d_src || !job->d_coef) return refuse_batch("null pointer");
  const ilcc_jpeg_fdct_batch_job J = *job;
  if (!jpeg_laid_out(*J.layout)) return refuse_batch("the layout's block counts and offsets are not ilcc_jpeg_layout's");
  const ilcc_jpeg_info& I = *J.layout;
  for (int c = 0; c < I.n_components; ++c) {
    if (I.comp[c].quant_index > 1) return refuse_batch("quantisation table index outside 0 .. 1");
    for (int k = 0; k < 64; ++k)
      if (I.quant[I.comp[c].quant_index][k] < 1 || I.quant[I.comp[c].quant_index][k] > 255) return refuse_batch("quantisation entry outside 1 .. 255");
  }
  const int bpp = I.n_components == 1 ? 1 : 3;
  if (J.encoding != (bpp == 1 ? ILCC_ENCODING_MONO8 : ILCC_ENCODING_BGR8))
    return refuse_batch("the encoding does not fit the components: mono8 for 1, bgr8 for 3");
  if (J.n_images > 65535u) return refuse_batch("more than 65535 images");
  if ((int64_t)J.src_stride < (int64_t)bpp * I.width) return refuse_batch("src_stride is shorter than a row");
  if (J.image_pitch < (uint64_t)J.src_stride * (uint64_t)(I.height - 1) + (uint64_t)bpp * (uint64_t)I.width)
    return refuse_batch("image_pitch is less than an image");
  if (J.coef_pitch < I.coef_count || (J.coef_pitch & 7u)) return refuse_batch("coef_pitch must hold coef_count and be a multiple of 8");
  if ((uintptr_t)J.d_coef & 15u) return refuse_batch("d_coef must be 16-byte aligned");
  const uint64_t per_image = ilcc_jpeg_fdct_scratch_bytes(J.layout);
  if (bpp == 3) {
    if (!J.d_scratch || ((uintptr_t)J.d_scratch & 15u)) return refuse_batch("d_scratch must be a 16-byte aligned device pointer");
    if (J.scratch_bytes < per_image * J.n_images) return refuse_batch("scratch_bytes is less than ilcc_jpeg_fdct_batch_scratch_bytes");
  }
  if (J.n_images == 0) return ILCC_OK;
  hipStream_t s = (hipStream_t)J.hip_stream;

  ColourArgs ca{};
  if (bpp == 3) {
    ColourBatchArgs cb;
    cb.image0 = ca = colour_args(I, J.d_src, J.src_stride, (uint8_t*)J.d_scratch);
    cb.src_pitch = J.image_pitch;
    cb.plane_pitch = per_image;
    const int rows = I.comp[0].v == 2 ? ca.plane_h / 2 : ca.plane_h;
    const dim3 block(kColTx, kColTy);
    const dim3 grid((ca.plane_w + kColTx * kColQuad - 1) / (kColTx * kColQuad), (rows + kColTy - 1) / kColTy, J.n_images);
    if (I.comp[0].h == 1) hipLaunchKernelGGL(k14b_colour_downsample<k444>, grid, block, 0, s, cb);
    else if (I.comp[0].v == 1) hipLaunchKernelGGL(k14b_colour_downsample<k422>, grid, block, 0, s, cb);
    else hipLaunchKernelGGL(k14b_colour_downsample<k420>, grid, block, 0, s, cb);
  }
  FdctBatchArgs fb{};
  fdct_args_all(I, J.d_src, J.src_stride, &ca, J.d_coef, fb.comp);
  int32_t rows = 0;
  for (int c = 0; c < 3; ++c) {
    fb.first_row[c] = c < I.n_components ? rows : INT32_MAX;   // a gray batch: no row of the grid reaches components 1 and 2
    if (c < I.n_components) rows += I.comp[c].blocks_h;
  }
  fb.src_pitch = bpp == 1 ? J.image_pitch : per_image;
  fb.coef_pitch = J.coef_pitch;
  const dim3 grid((I.comp[0].blocks_w + kBlocksPerGroup - 1) / kBlocksPerGroup, rows, J.n_images);   // luma is the widest component
  hipLaunchKernelGGL(k14b_fdct_quant, grid, dim3(kFdctThreads), 0, s, fb);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_global_error(std::string("k14b launch: ") + hipGetErrorString(e));
    return ILCC_HIP_ERROR;
  }
  return ILCC_OK;
}
