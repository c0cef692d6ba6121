// What csrc/jpeg_entropy.cpp shares with csrc/jpeg_scan_prepare.cpp: the Huffman table as the header reader builds it, and the
// header reader itself.  Plain C++17, no HIP.
#ifndef ILCC_JPEG_TABLES_H_
#define ILCC_JPEG_TABLES_H_

#include <cstdint>
#include <cstring>

#include "ilcc_jpeg.h"

namespace ilcc {

constexpr int kJpegLookBits = 9;

struct JpegHuffman {
  bool defined = false;
  uint8_t values[256];
  int32_t maxcode[17];                   // largest code of each length, -1: none
  int32_t first[17];                     // index in values[] of the first code of each length, minus that code
  uint16_t look[1 << kJpegLookBits];     // kJpegLookBits-bit prefix -> length << 8 | symbol, 0: longer than kJpegLookBits

  // counts[16] and the symbols behind them; false: more codes of a length than that length has
  bool define(const uint8_t* counts, const uint8_t* symbols, int total) {
    std::memcpy(values, symbols, (size_t)total);
    std::memset(look, 0, sizeof(look));
    int32_t code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
      const int n = counts[len - 1];
      first[len] = k - code;
      if (code + n > (1 << len)) return false;
      for (int i = 0; i < n; ++i, ++k, ++code)
        if (len <= kJpegLookBits)
          for (int fill = 0; fill < (1 << (kJpegLookBits - len)); ++fill)
            look[(code << (kJpegLookBits - len)) | fill] = (uint16_t)((len << 8) | values[k]);
      maxcode[len] = n ? code - 1 : -1;
      code <<= 1;
    }
    defined = true;
    return true;
  }
};

struct JpegTables {
  JpegHuffman dc[4], ac[4];
};

// The segments in front of the scan: fills *info, and the Huffman tables when `tables` is given.  The refusals and their texts
// are ilcc_jpeg_parse's.
int32_t jpeg_read_headers(const uint8_t* jpg, uint64_t bytes, ilcc_jpeg_info* info, JpegTables* tables);

}  // namespace ilcc

#endif
