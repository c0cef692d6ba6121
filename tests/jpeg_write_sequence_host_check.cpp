// Stand-alone check of ilcc_jpeg_write_headers (csrc/jpeg_entropy_enc.cpp), built by tests/test_jpeg_write_sequence_cpu.py with
// -fsanitize=address,undefined from this file, csrc/jpeg_entropy_enc.cpp and csrc/jpeg_entropy.cpp only.  For every accepted
// sampling, several sizes and restart intervals: the headers in a buffer of exactly their size are the first bytes of
// ilcc_jpeg_entropy_encode's file, headers + the file's scan + EOI is the file, and every capacity below the size is refused
// with ILCC_CAPACITY without a byte written past it (the buffer is a heap block of exactly `cap` bytes: ASan sees one more).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ilcc_hip.h"
#include "ilcc_jpeg_write.h"
#include "ilcc_jpeg_write_sequence.h"

static int fail(const char* what, int a = 0, int b = 0) {
  std::printf("FAILED: %s (%d, %d)\n", what, a, b);
  return 1;
}

int main() {
  const int samplings[4][3] = {{1, 1, 1}, {3, 1, 1}, {3, 2, 1}, {3, 2, 2}};
  const int sizes[4][2] = {{1, 1}, {17, 33}, {64, 48}, {257, 9}};
  const int restarts[3] = {0, 1, 7};
  int checked = 0;
  for (const auto& s : samplings)
    for (const auto& wh : sizes)
      for (int restart : restarts)
        for (int quality : {1, 50, 100}) {
          ilcc_jpeg_info I;
          if (ilcc_jpeg_write_info(wh[0], wh[1], s[0], s[1], s[2], quality, restart, &I) != ILCC_OK) return fail("write_info", wh[0], wh[1]);
          uint64_t need = 0;
          if (ilcc_jpeg_write_headers(&I, nullptr, 0, &need) != ILCC_CAPACITY || need != 0) return fail("cap 0 is ILCC_CAPACITY with 0 bytes");
          std::vector<uint8_t> big(2048);
          if (ilcc_jpeg_write_headers(&I, big.data(), big.size(), &need) != ILCC_OK || need == 0 || need > 629) return fail("headers", (int)need);
          for (uint64_t cap = need > 40 ? need - 40 : 0; cap <= need; ++cap) {
            uint8_t* exact = (uint8_t*)std::malloc(cap ? cap : 1);
            uint64_t got = 99;
            const int32_t st = ilcc_jpeg_write_headers(&I, cap ? exact : nullptr, cap, &got);
            const bool ok = cap == need ? (st == ILCC_OK && got == need && std::memcmp(exact, big.data(), need) == 0) : (st == ILCC_CAPACITY && got == 0);
            std::free(exact);
            if (!ok) return fail("capacity", (int)cap, (int)need);
          }
          // a file of this info: a few non-zero coefficients
          std::vector<int16_t> coef(I.coef_count, 0);
          for (uint64_t k = 0; k < I.coef_count; k += 64) {
            coef[k] = (int16_t)((k / 64) % 50);
            coef[k + 1 + (k / 64) % 63] = (int16_t)(1023 - (k / 64) % 7);
          }
          std::vector<uint8_t> file(ilcc_jpeg_file_bound(&I));
          uint64_t n = 0;
          if (ilcc_jpeg_entropy_encode(&I, coef.data(), file.data(), file.size(), &n) != ILCC_OK) return fail("entropy_encode");
          if (n < need + 2 || std::memcmp(file.data(), big.data(), need) != 0) return fail("the file does not start with the headers");
          if (file[n - 2] != 0xFF || file[n - 1] != 0xD9) return fail("the file does not end with EOI");
          ++checked;
        }
  ilcc_jpeg_info I;
  uint64_t n = 7;
  uint8_t room[700];
  if (ilcc_jpeg_write_headers(nullptr, room, sizeof(room), &n) != ILCC_BAD_ARGUMENT) return fail("null info");
  ilcc_jpeg_write_info(16, 16, 3, 2, 2, 90, 0, &I);
  if (ilcc_jpeg_write_headers(&I, room, sizeof(room), nullptr) != ILCC_BAD_ARGUMENT) return fail("null bytes");
  I.comp[1].dc_table = 2;
  if (ilcc_jpeg_write_headers(&I, room, sizeof(room), &n) != ILCC_BAD_ARGUMENT || n != 0) return fail("table index 2");
  std::printf("%d infos checked\n", checked);
  return 0;
}
