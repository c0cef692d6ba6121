// bayer_tap.h -- one pixel of a demosaiced Bayer frame, as include/ilcc_camera_image.h states it (OpenCV 3's scalar
// Bayer2RGB_ / Bayer2Gray_ behind cv_bridge): the clamp that makes the border, the site classification, colour and gray
// from the 3 x 3 raw neighbourhood, and the two ways K11 (csrc/k11_camera_image.hip) reads that neighbourhood from
// memory: a 4 x 4 window shared by the four taps of a bilinear sample, and a 6-column row for the four adjacent pixels
// a thread converts without a camera.  Plain inline functions, __host__ __device__ under
// hipcc, so that a host program (tests/bayer_host_check.cpp, under AddressSanitizer) runs exactly what the kernel
// runs.  No reader touches a byte outside [row * step, row * step + width) of any row.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define ILCC_BAYER_FN __host__ __device__ inline
#else
#define ILCC_BAYER_FN inline
#endif
#include <cstdint>

namespace ilcc {

// pattern = ilcc_image_encoding - ILCC_ENCODING_BAYER_RGGB8: the colours of pixels (0,0) (1,0) / (0,1) (1,1)
constexpr int kBayerRGGB = 0, kBayerBGGR = 1, kBayerGBRG = 2, kBayerGRBG = 3;
constexpr int kBayerMinSide = 3;   // a narrower or lower image has no interior pixel

// D(x, y) = I(clamp(x, 1, w - 2), clamp(y, 1, h - 2)): the border repeats its inner neighbour
ILCC_BAYER_FN int bayer_clamp(int v, int n) { return v < 1 ? 1 : (v > n - 2 ? n - 2 : v); }

ILCC_BAYER_FN bool bayer_green_site(int pattern, int x, int y) { return (((x + y) & 1) != 0) != (pattern >= kBayerGBRG); }

// the row's non-green sites are red (else blue)
ILCC_BAYER_FN bool bayer_red_row(int pattern, int y) { return (y & 1) == ((pattern == kBayerBGGR || pattern == kBayerGBRG) ? 1 : 0); }

// The 3 x 3 neighbourhood travels as three row triples t0, t1, t2 (rows y - 1, y, y + 1): left | centre << 8 | right << 16.
struct BayerSums {
  uint32_t c, lr, ud, diag;   // centre; left + right; up + down; the four diagonals
};

ILCC_BAYER_FN BayerSums bayer_sums(uint32_t t0, uint32_t t1, uint32_t t2) {
  BayerSums s;
  s.c = (t1 >> 8) & 255u;
  s.lr = (t1 & 255u) + ((t1 >> 16) & 255u);
  s.ud = ((t0 >> 8) & 255u) + ((t2 >> 8) & 255u);
  s.diag = (t0 & 255u) + ((t0 >> 16) & 255u) + (t2 & 255u) + ((t2 >> 16) & 255u);
  return s;
}

// B | G << 8 | R << 16
ILCC_BAYER_FN uint32_t bayer_bgr(uint32_t t0, uint32_t t1, uint32_t t2, bool green, bool red_row) {
  const BayerSums s = bayer_sums(t0, t1, t2);
  uint32_t g, row_colour, other;   // row_colour: of this row's non-green sites
  if (green) {
    g = s.c;
    row_colour = (s.lr + 1u) >> 1;
    other = (s.ud + 1u) >> 1;
  } else {
    g = (s.lr + s.ud + 2u) >> 2;
    row_colour = s.c;
    other = (s.diag + 2u) >> 2;
  }
  const uint32_t r = red_row ? row_colour : other, b = red_row ? other : row_colour;
  return b | (g << 8) | (r << 16);
}

// Y from the raw sums (not the gray of bayer_bgr: one rounding instead of two)
ILCC_BAYER_FN uint32_t bayer_gray(uint32_t t0, uint32_t t1, uint32_t t2, bool green, bool red_row) {
  constexpr uint32_t cR = 4899u, cG = 9617u, cB = 1868u;
  const BayerSums s = bayer_sums(t0, t1, t2);
  const uint32_t c_row = red_row ? cR : cB, c_other = red_row ? cB : cR;
  if (green) return (2u * cG * s.c + c_row * s.lr + c_other * s.ud + 16384u) >> 15;
  return (4u * c_row * s.c + cG * (s.lr + s.ud) + c_other * s.diag + 32768u) >> 16;
}

ILCC_BAYER_FN uint32_t bayer_value(bool gray, int pattern, int cx, int cy, uint32_t t0, uint32_t t1, uint32_t t2) {
  const bool green = bayer_green_site(pattern, cx, cy), red_row = bayer_red_row(pattern, cy);
  return gray ? bayer_gray(t0, t1, t2, green, red_row) : bayer_bgr(t0, t1, t2, green, red_row);
}

// ---------------------------------------------------------------- the 4 x 4 window of a bilinear sample
// A w x h frame (w, h >= 3) whose rows lie `step` bytes apart.  The taps (x0 .. x0 + 1, y0 .. y0 + 1) have clamped centres in columns bx + 1 .. bx + 2 and rows by + 1 .. by + 2, so
// their neighbourhoods lie in columns bx .. bx + 3 and rows by .. by + 3; the part of that beyond the frame (possible
// only in the last column and row of the window) is not read and not used.
struct BayerWindow {
  int bx, by;
  uint32_t row[4];   // row[r]: the bytes of columns bx .. bx + 3 of row by + r, the lowest byte first
};

ILCC_BAYER_FN uint32_t bayer_load4(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);   // little-endian; any alignment
  return v;
}

ILCC_BAYER_FN BayerWindow bayer_window(const uint8_t* src, int64_t step, int w, int h, int x0, int y0) {
  BayerWindow W;
  W.bx = bayer_clamp(x0, w) - 1;
  W.by = bayer_clamp(y0, h) - 1;
  const bool whole = W.bx + 3 < w;
  const uint8_t* p = src + (int64_t)W.by * step + W.bx;
  for (int r = 0; r < 4; ++r, p += step) {
    uint32_t v = 0;
    if (W.by + r < h) {
      if (whole) v = bayer_load4(p);
      else v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);   // bx + 2 <= w - 1 always
    }
    W.row[r] = v;
  }
  return W;
}

// tap (x, y), one of the window's four: D(x, y) as Y (gray) or B | G << 8 | R << 16; 0 outside the frame (BORDER_CONSTANT)
ILCC_BAYER_FN uint32_t bayer_window_tap(const BayerWindow& W, int w, int h, int pattern, bool gray, int x, int y) {
  if ((uint32_t)x >= (uint32_t)w || (uint32_t)y >= (uint32_t)h) return 0;
  const int cx = bayer_clamp(x, w), cy = bayer_clamp(y, h);
  const bool low = cy - W.by == 1;          // centre in window row 1, else 2
  const int sh = 8 * (cx - W.bx - 1);       // 0 or 8
  const uint32_t t0 = ((low ? W.row[0] : W.row[1]) >> sh) & 0xFFFFFFu;
  const uint32_t t1 = ((low ? W.row[1] : W.row[2]) >> sh) & 0xFFFFFFu;
  const uint32_t t2 = ((low ? W.row[2] : W.row[3]) >> sh) & 0xFFFFFFu;
  return bayer_value(gray, pattern, cx, cy, t0, t1, t2);
}

// ---------------------------------------------------------------- the rows of four adjacent pixels, no camera
// Pixels j0 .. j0 + n - 1 (n <= 4, j0 + n <= w) of one row have clamped centres in columns lo + 1 .. lo + 4, lo =
// clamp(j0) - 1.  bayer_row6: the bytes of columns lo .. lo + 5 of one row as a 48-bit word (0 beyond the frame): one
// dword where an aligned one lies wholly inside both that span and the row, bytes for the rest.
ILCC_BAYER_FN uint64_t bayer_row6(const uint8_t* row, int w, int lo) {
  const uint8_t* p = row + lo;
  const int off = (int)((0u - (uint32_t)(uintptr_t)p) & 3u);   // distance to the next 4-byte boundary
  const bool wide = off <= 2 && lo + off + 3 < w;
  uint64_t v = 0;
  if (wide) v = (uint64_t)*reinterpret_cast<const uint32_t*>(p + off) << (8 * off);
  for (int c = 0; c < 6; ++c)
    if (lo + c < w && !(wide && c >= off && c < off + 4)) v |= (uint64_t)p[c] << (8 * c);
  return v;
}

// pixel (x, y) of those four from the rows cy - 1, cy, cy + 1 (cy = clamp(y)) read by bayer_row6 with the same lo
ILCC_BAYER_FN uint32_t bayer_row6_pixel(uint64_t r0, uint64_t r1, uint64_t r2, int lo, int w, int h, int pattern, bool gray, int x, int y) {
  const int cx = bayer_clamp(x, w), cy = bayer_clamp(y, h);
  const int sh = 8 * (cx - lo - 1);         // 0, 8, 16 or 24
  return bayer_value(gray, pattern, cx, cy, (uint32_t)(r0 >> sh) & 0xFFFFFFu, (uint32_t)(r1 >> sh) & 0xFFFFFFu,
                     (uint32_t)(r2 >> sh) & 0xFFFFFFu);
}

}  // namespace ilcc
