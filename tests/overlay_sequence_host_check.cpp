// Stand-alone check of csrc/overlay_sequence_host.cpp (include/ilcc_overlay_sequence.h), built with AddressSanitizer and UBSan by
// tests/test_overlay_sequence_cpu.py from that file and this one alone.  The three JPEG size functions the file adds up live in
// HIP translation units of the library; here they are stand-ins with sizes that are NOT multiples of 256, so that every rounding of
// the formula shows: the test restates the same stand-ins in python.
//   overlay_sequence_host_check cases.txt      cases.txt: "n" then n lines "width height out_bytes_per_image"
// prints one line "width height out bytes" per case, then the default parameters.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ilcc_jpeg_write.h"
#include "ilcc_jpeg_write_sequence.h"
#include "ilcc_overlay_sequence.h"

extern "C" {

// 4:2:0: MCUs of 16 x 16 pixels, six blocks each
int32_t ilcc_jpeg_write_info(int32_t width, int32_t height, int32_t n_components, int32_t sampling_h, int32_t sampling_v, int32_t, int32_t,
                             ilcc_jpeg_info* out) {
  if (width < 1 || height < 1 || width > 65535 || height > 65535 || n_components != 3 || sampling_h != 2 || sampling_v != 2 || !out) return ILCC_BAD_ARGUMENT;
  std::memset(out, 0, sizeof(*out));
  out->width = width;
  out->height = height;
  out->n_components = 3;
  const uint64_t mcus = (uint64_t)((width + 15) / 16) * (uint64_t)((height + 15) / 16);
  out->coef_count = mcus * 6 * 64;
  return ILCC_OK;
}

uint64_t ilcc_jpeg_fdct_scratch_bytes(const ilcc_jpeg_info* info) { return info->coef_count + 3; }

// refuses, as K17 does, an image whose worst-case scan has 2^32 bits or more
uint64_t ilcc_jpeg_huffman_encode_scratch_bytes(const ilcc_jpeg_info* layout, uint32_t n_images, uint64_t out_cap) {
  if (layout->coef_count * 16 * 2 >= (1ull << 32)) return 0;
  return 256 * ((out_cap + 4096ull * n_images + layout->coef_count / 8) / 256 + 1);
}

}  // extern "C"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n = 0;
  if (std::fscanf(f, "%d", &n) != 1 || n < 0) return 2;
  for (int k = 0; k < n; ++k) {
    long long w = 0, h = 0;
    unsigned long long out = 0;
    if (std::fscanf(f, "%lld %lld %llu", &w, &h, &out) != 3) return 2;
    std::printf("%lld %lld %llu %llu\n", w, h, out, (unsigned long long)ilcc_overlay_sequence_bytes((int32_t)w, (int32_t)h, out));
  }
  std::fclose(f);
  ilcc_overlay_sequence_params sp;
  std::memset(&sp, 0xEE, sizeof(sp));
  ilcc_default_overlay_sequence_params(&sp);
  ilcc_default_overlay_sequence_params(nullptr);
  std::printf("defaults %u %u %u %u %u %u %llu %llu %llu %llu %llu size %zu %zu\n", sp.first, sp.stride, sp.max_scans, sp.route, sp.keep_pixels, sp.reserved,
              (unsigned long long)sp.max_dt_ns, (unsigned long long)sp.staging_bytes, (unsigned long long)sp.image_bytes, (unsigned long long)sp.device_bytes,
              (unsigned long long)sp.out_bytes_per_image, sizeof(ilcc_overlay_sequence_params), sizeof(ilcc_overlay_record));
  return 0;
}
