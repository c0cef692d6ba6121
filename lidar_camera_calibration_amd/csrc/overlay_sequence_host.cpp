// overlay_sequence_host.cpp -- the host-only layer of include/ilcc_overlay_sequence.h: the device bytes one paired scan takes in
// ilcc_bag_pcd2image_all_pairs, which cuts its batches with them, and the chain's default parameters.  Plain C++ without HIP: it
// also builds alone, under sanitizers, for tests/test_overlay_sequence_cpu.py (which supplies the three JPEG size functions it
// calls; in the library they are jpeg_write_host.cpp's, K14's and K17's).
#include <cstring>

#include "ilcc_jpeg_write.h"
#include "ilcc_jpeg_write_sequence.h"
#include "ilcc_overlay_sequence.h"

namespace {

constexpr uint64_t kDefaultStagingBytes = 256ull << 20, kDefaultImageBytes = 512ull << 20, kDefaultDeviceBytes = 1ull << 30;
constexpr uint64_t kDefaultMaxDtNs = 50000000ull;

uint64_t up(uint64_t x) { return (x + 255u) & ~(uint64_t)255u; }
uint64_t up16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }

}  // namespace

extern "C" {

uint64_t ilcc_overlay_sequence_bytes(int32_t width, int32_t height, uint64_t out_bytes_per_image) {
  ilcc_jpeg_info I;
  if (ilcc_jpeg_write_info(width, height, 3, 2, 2, 95, 0, &I) != ILCC_OK) return 0;   // the sizes do not depend on the quality
  const uint64_t pixels = (uint64_t)width * (uint64_t)height;
  if (out_bytes_per_image > (1ull << 40)) return 0;
  const uint64_t out = up16(out_bytes_per_image ? out_bytes_per_image : pixels);
  const uint64_t k17 = ilcc_jpeg_huffman_encode_scratch_bytes(&I, 1, out);
  if (k17 == 0) return 0;
  return up(3 * pixels) + up(4 * pixels) + up(I.coef_count * sizeof(int16_t)) + up(ilcc_jpeg_fdct_scratch_bytes(&I)) + up(out) + 256 + k17;
}

void ilcc_default_overlay_sequence_params(ilcc_overlay_sequence_params* sp) {
  if (!sp) return;
  std::memset(sp, 0, sizeof(*sp));
  sp->stride = 1;
  sp->max_dt_ns = kDefaultMaxDtNs;
  sp->staging_bytes = kDefaultStagingBytes;
  sp->image_bytes = kDefaultImageBytes;
  sp->device_bytes = kDefaultDeviceBytes;
}

}  // extern "C"
