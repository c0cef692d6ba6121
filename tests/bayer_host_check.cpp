// Stand-alone check of csrc/bayer_tap.h, the code K11 runs per tap, on the host under AddressSanitizer and UBSan
// (tests/test_bayer_cpu.py builds and feeds it).  Usage: bayer_host_check cases.bin
// cases.bin: per case  int32 pattern, w, h | w*h raw bytes | w*h*3 expected B,G,R | w*h expected Y  (tests/bayer_ref.py).
// Every raw image is read from a heap block of exactly w*h bytes, so a read past any end is an error, and from a second
// block in which the rows lie w + 3 bytes apart and start one byte into it, for other alignments of the dword loads.
// Checked against the expectations: the four taps of the window of every sample position -3 .. w+1 x -3 .. h+1, so every
// tap position of -3 .. w+2 x -3 .. h+2 in each of its four roles (0 outside the frame), and the 6-column rows of every
// quad of every row.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bayer_tap.h"

using namespace ilcc;

namespace {

struct Case {
  int32_t pattern, w, h;
  std::vector<uint8_t> bgr, gray;
};

long failures = 0;

void expect(uint32_t got, uint32_t want, const Case& c, const char* what, int x, int y, bool gray) {
  if (got == want) return;
  if (++failures <= 20)
    std::fprintf(stderr, "pattern %d %d x %d %s %s at (%d, %d): got %06x, expected %06x\n", c.pattern, c.w, c.h, what, gray ? "gray" : "colour",
                 x, y, got, want);
}

uint32_t expected(const Case& c, bool gray, int x, int y) {
  if (x < 0 || y < 0 || x >= c.w || y >= c.h) return 0;
  const size_t at = (size_t)y * c.w + x;
  if (gray) return c.gray[at];
  return (uint32_t)c.bgr[3 * at] | ((uint32_t)c.bgr[3 * at + 1] << 8) | ((uint32_t)c.bgr[3 * at + 2] << 16);
}

void check(const Case& c, const uint8_t* src, int64_t step) {
  const int w = c.w, h = c.h, p = c.pattern;
  for (int g = 0; g < 2; ++g) {
    const bool gray = g == 1;
    for (int y0 = -3; y0 <= h + 1; ++y0)
      for (int x0 = -3; x0 <= w + 1; ++x0) {
        const BayerWindow W = bayer_window(src, step, w, h, x0, y0);
        for (int k = 0; k < 4; ++k) {
          const int x = x0 + (k & 1), y = y0 + (k >> 1);
          expect(bayer_window_tap(W, w, h, p, gray, x, y), expected(c, gray, x, y), c, "window tap", x, y, gray);
        }
      }
    for (int i = 0; i < h; ++i) {
      const uint8_t* row = src + (int64_t)(bayer_clamp(i, h) - 1) * step;
      for (int j0 = 0; j0 < w; j0 += 4) {
        const int lo = bayer_clamp(j0, w) - 1;
        const uint64_t r0 = bayer_row6(row, w, lo), r1 = bayer_row6(row + step, w, lo), r2 = bayer_row6(row + 2 * step, w, lo);
        for (int k = 0; k < 4 && j0 + k < w; ++k)
          expect(bayer_row6_pixel(r0, r1, r2, lo, w, h, p, gray, j0 + k, i), expected(c, gray, j0 + k, i), c, "quad pixel", j0 + k, i, gray);
      }
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::fprintf(stderr, "can not open %s\n", argv[1]);
    return 2;
  }
  long cases = 0, pixels = 0;
  for (;;) {
    Case c;
    int32_t head[3];
    const size_t got = std::fread(head, sizeof(int32_t), 3, f);
    if (got == 0) break;
    if (got != 3 || head[0] < 0 || head[0] > 3 || head[1] < kBayerMinSide || head[2] < kBayerMinSide || head[1] > 4096 || head[2] > 4096) {
      std::fprintf(stderr, "bad case header\n");
      return 2;
    }
    c.pattern = head[0];
    c.w = head[1];
    c.h = head[2];
    const size_t n = (size_t)c.w * c.h;
    uint8_t* raw = (uint8_t*)std::malloc(n);   // exactly w * h bytes
    c.bgr.resize(3 * n);
    c.gray.resize(n);
    if (!raw || std::fread(raw, 1, n, f) != n || std::fread(c.bgr.data(), 1, 3 * n, f) != 3 * n || std::fread(c.gray.data(), 1, n, f) != n) {
      std::fprintf(stderr, "truncated case\n");
      return 2;
    }
    check(c, raw, c.w);
    // pitched: the last row ends with the block, the first starts one byte in
    const int64_t step = c.w + 3;
    const size_t pitched_bytes = 1 + (size_t)(c.h - 1) * step + c.w;
    uint8_t* pitched = (uint8_t*)std::malloc(pitched_bytes);
    if (!pitched) return 2;
    std::memset(pitched, 0xAB, pitched_bytes);
    for (int r = 0; r < c.h; ++r) std::memcpy(pitched + 1 + r * step, raw + (size_t)r * c.w, c.w);
    check(c, pitched + 1, step);
    std::free(pitched);
    std::free(raw);
    ++cases;
    pixels += (long)n;
  }
  std::fclose(f);
  if (failures) {
    std::fprintf(stderr, "%ld mismatches\n", failures);
    return 1;
  }
  std::printf("%ld cases, %ld pixels: every tap, window and quad reproduced\n", cases, pixels);
  return 0;
}
