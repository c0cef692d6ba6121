// K13b -- K13 on a batch of JPEG images of one geometry (include/ilcc_jpeg_sequence.h): the coefficients of n images, each
// with its own quantisation tables, -> n images of pixels, in TWO launches for a colour batch and ONE for a gray batch,
// whatever n is.  The stage bodies are K13's own (csrc/k13_stages.h), compiled with the same flags: every byte equals what
// ilcc_jpeg_idct_device writes for that image alone.
//
// k13b_idct: one launch for all components of all images.  The thread-to-data map inside a workgroup is K13's (256 threads =
//   32 blocks of eight lanes side by side in one block row, a 16-byte load per lane, the transposes in registers).  The grid:
//   z   the image.  Images differ only in base addresses (coefficients, tables, planes), which are scalar arithmetic on
//       blockIdx.z; n <= 65535 is the grid's limit and the entry's.
//   y   (component, block row) flattened: rows [0, h0) are luma's, [h0, h0 + h1) Cb's, the rest Cr's.  Two compares against
//       kernel arguments find the component; they are wave-uniform, so the component's offsets, widths and strides stay in
//       scalar registers.  Flattening into y rather than giving the component its own grid dimension launches no workgroup
//       for block rows a subsampled chroma plane does not have (4:2:0: half the luma's rows).
//   x   the 32-block group, sized for the widest component (luma).  A group that starts past the end of a narrower
//       component's row leaves as a whole -- the test is uniform over the workgroup, so no lane leaves before the exchanges;
//       inside a live group a block past the row's end is computed on zeros and not stored, as in K13.  With 4:2:0 a quarter
//       of the chroma rows' workgroups leave at once (two scalar compares and a branch each), which keeps the launch count
//       at one.
//   A 1920 x 1200 4:2:0 frame is 8 x (150 + 75 + 75) = 2400 workgroups an image, of 4 wavefronts each: a batch gives the
//   chip's 1024 SIMDs many rounds of work in one launch, where K13's three launches per image each end in a partial round.
//   The quantisation row comes from device memory -- image m's table c is at d_quant + (3 m + c) * 64 -- as one 16-byte load
//   per lane where K13 reads its by-value argument: a by-value table per image would mean a launch per image.  The eight
//   rows of a table are 128 contiguous bytes which every block of the workgroup reads: after the first wavefront they hit in
//   cache.
// k13b_upsample_colour: K13's map (64 x 4 threads over 256 x 4 pixels) with the image as blockIdx.z.  The mode is one template
//   choice per batch since the geometry is shared.  Image m's planes lie at d_scratch + m * ilcc_jpeg_scratch_bytes(layout),
//   each padded to whole blocks and on a 256-byte boundary as in K13, so the luma dword load and the clamped chroma reads
//   stay inside the image's own planes.
#include <hip/hip_runtime.h>

#include <string>

#include "host_util.h"
#include "ilcc_hip.h"
#include "ilcc_jpeg_sequence.h"
#include "jpeg_entropy.h"
#include "k13_stages.h"

namespace ilcc {

struct IdctBatchComponent {
  uint64_t coef_offset;      // of the component's first block in an image's coefficients, int16
  uint64_t dst_offset;       // of the component's plane in an image's part of the destination, bytes
  int64_t dst_stride;
  int32_t blocks_w;
  int32_t first_row;         // of the component in the flattened blockIdx.y
  int32_t clip_w, clip_h;    // nothing is stored at x >= clip_w or y >= clip_h
};

struct IdctBatchArgs {
  const int16_t* coef;
  uint64_t coef_pitch;       // int16 between images
  const uint16_t* quant;     // [n][3][64]
  uint8_t* dst;
  uint64_t dst_pitch;        // bytes between images
  IdctBatchComponent comp[3];
};

__global__ __launch_bounds__(kIdctThreads) void k13b_idct(IdctBatchArgs a) {
  const int row = blockIdx.y;
  const int c = (row >= a.comp[1].first_row ? 1 : 0) + (row >= a.comp[2].first_row ? 1 : 0);   // wave-uniform
  const IdctBatchComponent& K = c == 0 ? a.comp[0] : c == 1 ? a.comp[1] : a.comp[2];
  if ((int)(blockIdx.x * kBlocksPerGroup) >= K.blocks_w) return;   // the whole workgroup: this component's rows are narrower
  const uint64_t m = blockIdx.z;
  const int lane8 = threadIdx.x & 7;
  const int bx = blockIdx.x * kBlocksPerGroup + (threadIdx.x >> 3);
  const int by = row - K.first_row;
  const bool live = bx < K.blocks_w;
  int32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    const int16_t* crow = a.coef + m * a.coef_pitch + K.coef_offset + ((int64_t)by * K.blocks_w + bx) * 64 + lane8 * 8;
    const uint16_t* qrow = a.quant + (m * 3 + (uint64_t)c) * 64 + lane8 * 8;
    idct_dequantise(*reinterpret_cast<const uint4*>(crow), *reinterpret_cast<const uint4*>(qrow), v);
  }
  idct_block(v, lane8, live, bx, by, a.dst + m * a.dst_pitch + K.dst_offset, K.dst_stride, K.clip_w, K.clip_h);
}

struct ColourBatchArgs {
  ColourArgs image0;         // image 0's planes and destination
  uint64_t plane_pitch;      // bytes between the images' planes
  uint64_t dst_pitch;
};

template <int MODE>
__global__ __launch_bounds__(kColTx* kColTy) void k13b_upsample_colour(ColourBatchArgs b) {
  const int x0 = (blockIdx.x * kColTx + threadIdx.x) * kColQuad;
  const int y = blockIdx.y * kColTy + threadIdx.y;
  if (x0 >= b.image0.width || y >= b.image0.height) return;
  const uint64_t m = blockIdx.z;
  ColourArgs a = b.image0;
  a.y += m * b.plane_pitch;
  a.cb += m * b.plane_pitch;
  a.cr += m * b.plane_pitch;
  a.dst += m * b.dst_pitch;
  upsample_colour_quad<MODE>(a, x0, y);
}

namespace {

int32_t refuse(const std::string& what) {
  set_global_error("ilcc_jpeg_idct_batch_device: " + what);
  return ILCC_BAD_ARGUMENT;
}

uint64_t image_scratch_bytes(const ilcc_jpeg_info& I) { return jpeg_plane_bytes(I.comp[0]) + jpeg_plane_bytes(I.comp[1]) + jpeg_plane_bytes(I.comp[2]); }

}  // namespace
}  // namespace ilcc

extern "C" uint64_t ilcc_jpeg_batch_scratch_bytes(const ilcc_jpeg_info* layout, uint32_t n_images) {
  using namespace ilcc;
  if (!layout || layout->n_components != 3 || !jpeg_laid_out(*layout)) return 0;
  return image_scratch_bytes(*layout) * (uint64_t)n_images;
}

extern "C" int32_t ilcc_jpeg_idct_batch_device(const ilcc_jpeg_info* layout, const uint16_t* d_quant, const int16_t* d_coef, uint64_t coef_pitch,
                                               uint32_t n_images, void* d_dst, uint64_t dst_pitch, int32_t dst_stride, void* d_scratch,
                                               uint64_t scratch_bytes, void* hip_stream) {
  using namespace ilcc;
  if (!layout || !d_quant || !d_coef || !d_dst) return refuse("null pointer");
  if (!jpeg_laid_out(*layout)) return refuse("the layout's block counts and offsets are not ilcc_jpeg_layout's");
  const ilcc_jpeg_info& I = *layout;
  const int bpp = I.n_components == 1 ? 1 : 3;
  if (n_images > 65535u) return refuse("more than 65535 images");
  if (coef_pitch < I.coef_count || (coef_pitch & 7u)) return refuse("coef_pitch must hold coef_count and be a multiple of 8");
  if ((uintptr_t)d_coef & 15u) return refuse("d_coef must be 16-byte aligned");
  if ((uintptr_t)d_quant & 15u) return refuse("d_quant must be 16-byte aligned");
  if ((int64_t)dst_stride < (int64_t)bpp * I.width) return refuse("dst_stride is shorter than a row");
  if (dst_pitch < (uint64_t)dst_stride * (uint64_t)I.height) return refuse("dst_pitch is less than dst_stride * height");
  const uint64_t per_image = bpp == 3 ? image_scratch_bytes(I) : 0;
  if (bpp == 3) {
    if (!d_scratch || ((uintptr_t)d_scratch & 15u)) return refuse("d_scratch must be a 16-byte aligned device pointer");
    if (scratch_bytes < per_image * n_images) return refuse("scratch_bytes is less than ilcc_jpeg_batch_scratch_bytes");
  }
  if (n_images == 0) return ILCC_OK;
  hipStream_t s = (hipStream_t)hip_stream;

  IdctBatchArgs a{};
  a.coef = d_coef;
  a.coef_pitch = coef_pitch;
  a.quant = d_quant;
  int32_t rows = 0;
  uint64_t plane_at = 0;
  for (int c = 0; c < 3; ++c) {
    IdctBatchComponent& K = a.comp[c];
    K.first_row = rows;
    if (c >= I.n_components) {   // a gray batch: no row of the grid reaches components 1 and 2
      K.first_row = INT32_MAX;
      continue;
    }
    K.coef_offset = I.comp[c].coef_offset;
    K.blocks_w = I.comp[c].blocks_w;
    if (bpp == 1) {   // straight into the image, clipped at its right and bottom edge
      K.dst_offset = 0;
      K.dst_stride = dst_stride;
      K.clip_w = I.width;
      K.clip_h = I.height;
    } else {          // whole padded planes: nothing clipped
      K.dst_offset = plane_at;
      K.dst_stride = 8 * I.comp[c].blocks_w;
      K.clip_w = 8 * I.comp[c].blocks_w;
      K.clip_h = 8 * I.comp[c].blocks_h;
      plane_at += jpeg_plane_bytes(I.comp[c]);
    }
    rows += I.comp[c].blocks_h;
  }
  a.dst = bpp == 1 ? (uint8_t*)d_dst : (uint8_t*)d_scratch;
  a.dst_pitch = bpp == 1 ? dst_pitch : per_image;
  const dim3 grid((I.comp[0].blocks_w + kBlocksPerGroup - 1) / kBlocksPerGroup, rows, n_images);   // luma is the widest component
  hipLaunchKernelGGL(k13b_idct, grid, dim3(kIdctThreads), 0, s, a);

  if (bpp == 3) {
    ColourBatchArgs b;
    b.image0 = colour_geometry(I, dst_stride);
    b.image0.y = (const uint8_t*)d_scratch;
    b.image0.cb = b.image0.y + jpeg_plane_bytes(I.comp[0]);
    b.image0.cr = b.image0.cb + jpeg_plane_bytes(I.comp[1]);
    b.image0.dst = (uint8_t*)d_dst;
    b.plane_pitch = per_image;
    b.dst_pitch = dst_pitch;
    const dim3 block(kColTx, kColTy);
    const dim3 cgrid((I.width + kColTx * kColQuad - 1) / (kColTx * kColQuad), (I.height + kColTy - 1) / kColTy, n_images);
    switch (chroma_mode(I)) {
      case kChroma444: hipLaunchKernelGGL(k13b_upsample_colour<kChroma444>, cgrid, block, 0, s, b); break;
      case kChroma422: hipLaunchKernelGGL(k13b_upsample_colour<kChroma422>, cgrid, block, 0, s, b); break;
      case kChroma422Replicate: hipLaunchKernelGGL(k13b_upsample_colour<kChroma422Replicate>, cgrid, block, 0, s, b); break;
      case kChroma420: hipLaunchKernelGGL(k13b_upsample_colour<kChroma420>, cgrid, block, 0, s, b); break;
      default: hipLaunchKernelGGL(k13b_upsample_colour<kChroma420Replicate>, cgrid, block, 0, s, b); break;
    }
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_global_error(std::string("k13b launch: ") + hipGetErrorString(e));
    return ILCC_HIP_ERROR;
  }
  return ILCC_OK;
}
