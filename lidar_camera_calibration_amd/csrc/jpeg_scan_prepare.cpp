// The host's part of K16 (include/ilcc_jpeg_huffman.h): one pass over a file's scan that removes the byte stuffing, cuts the bytes
// at the restart markers and hands out the Huffman tables in the form the kernel reads.  No Huffman code is decoded here.  Plain
// C++17: no HIP, no allocation, nothing read past `bytes`; it builds with csrc/jpeg_entropy.cpp alone
// (tests/jpeg_huffman_host_check.cpp links the two, under sanitizers).
#include <cstring>

#include "ilcc_hip.h"
#include "ilcc_jpeg_huffman.h"
#include "jpeg_entropy.h"
#include "jpeg_tables.h"

namespace {

using ilcc::jpeg_refuse;

constexpr uint64_t kMaxScanBytes = 1ull << 28;   // K16 counts a segment's bits in 32 bits

int32_t capacity(const char* what) {
  jpeg_refuse(what);
  return ILCC_CAPACITY;
}

// The scan's bytes from `at` on.  As in Bits::fill of csrc/jpeg_entropy.cpp any run of 0xFF bytes counts as one: followed by
// 0x00 it is the data byte 0xFF, followed by anything else it is a marker, followed by nothing the data has stopped.
struct Scan {
  const uint8_t* m;
  uint64_t n, at;

  // copies data bytes to out[*used ..] up to the next marker; -> the marker's code, 0: the data stopped; -1: out is full
  int32_t copy_segment(uint8_t* out, uint64_t cap, uint64_t* used) {
    while (at < n) {
      if (m[at] != 0xFF) {
        if (*used >= cap) return -1;
        out[(*used)++] = m[at++];
        continue;
      }
      uint64_t q = at + 1;
      while (q < n && m[q] == 0xFF) ++q;
      if (q >= n) break;
      at = q + 1;
      if (m[q] != 0x00) return m[q];
      if (*used >= cap) return -1;
      out[(*used)++] = 0xFF;
    }
    at = n;
    return 0;
  }
  // the next marker's code with the bytes in front of it skipped, 0: none (Bits::next_marker)
  int32_t next_marker() {
    while (at < n) {
      if (m[at] != 0xFF) {
        ++at;
        continue;
      }
      uint64_t q = at + 1;
      while (q < n && m[q] == 0xFF) ++q;
      if (q >= n) break;
      at = q + 1;
      if (m[q] != 0x00) return m[q];
    }
    at = n;
    return 0;
  }
};

void copy_table(const ilcc::JpegHuffman& from, ilcc_jpeg_huffman_table* to) {
  std::memcpy(to->look, from.look, sizeof(to->look));
  int used = 0;
  for (int len = 1; len <= 16; ++len) {
    to->maxcode[len] = from.maxcode[len];
    to->first[len] = from.first[len];
    if (from.maxcode[len] >= 0) used = from.first[len] + from.maxcode[len] + 1;
  }
  std::memcpy(to->values, from.values, (size_t)used);   // what is behind the last symbol stays 0
}

uint64_t mcu_count(const ilcc_jpeg_info& I) {
  return (uint64_t)(I.comp[0].blocks_w / I.comp[0].h) * (uint64_t)(I.comp[0].blocks_h / I.comp[0].v);
}

}  // namespace

extern "C" {

int32_t ilcc_jpeg_scan_bound(const ilcc_jpeg_info* info, uint64_t file_bytes, uint64_t* scan_bytes, uint32_t* n_segments) {
  if (!info || !scan_bytes || !n_segments) return jpeg_refuse("ilcc_jpeg_scan_bound: null argument");
  if (!ilcc::jpeg_laid_out(*info)) return jpeg_refuse("ilcc_jpeg_scan_bound: the info's block counts and offsets are not ilcc_jpeg_layout's");
  if (info->scan_offset > file_bytes) return jpeg_refuse("ilcc_jpeg_scan_bound: scan_offset is behind the end of the file");
  const uint64_t total = mcu_count(*info);
  const uint64_t interval = info->restart_interval > 0 ? (uint64_t)info->restart_interval : total;
  *scan_bytes = file_bytes - info->scan_offset;
  *n_segments = (uint32_t)((total + interval - 1) / interval);
  return ILCC_OK;
}

int32_t ilcc_jpeg_scan_prepare(const uint8_t* jpg, uint64_t bytes, const ilcc_jpeg_info* info, uint8_t* scan, uint64_t scan_cap,
                               uint64_t* scan_bytes, ilcc_jpeg_huffman_segment* segments, uint32_t segment_cap, uint32_t* n_segments,
                               ilcc_jpeg_huffman_tables* tables) {
  if (!jpg || !info || (!scan && scan_cap) || !scan_bytes || (!segments && segment_cap) || !n_segments || !tables)
    return jpeg_refuse("ilcc_jpeg_scan_prepare: null argument");
  *scan_bytes = 0;
  *n_segments = 0;
  ilcc_jpeg_info I;
  ilcc::JpegTables T;
  const int32_t st = ilcc::jpeg_read_headers(jpg, bytes, &I, &T);
  if (st != ILCC_OK) return st;
  if (std::memcmp(&I, info, sizeof(I)) != 0) return jpeg_refuse("ilcc_jpeg_scan_prepare: info is not ilcc_jpeg_parse's of these bytes");

  const uint64_t total = mcu_count(I);
  const uint64_t interval = I.restart_interval ? (uint64_t)I.restart_interval : total;
  const uint64_t rows = (total + interval - 1) / interval;
  if (rows > segment_cap) return capacity("segment table smaller than the scan's restart intervals");
  if (scan_cap > kMaxScanBytes - 1) scan_cap = kMaxScanBytes - 1;

  Scan s{jpg, bytes, I.scan_offset};
  uint64_t used = 0;
  int32_t m = 0;
  for (uint64_t k = 0; k < rows; ++k) {
    const uint64_t start = used;
    m = s.copy_segment(scan, scan_cap, &used);
    if (m < 0) return capacity(scan_cap == kMaxScanBytes - 1 ? "scan of 2^28 bytes or more" : "scan buffer smaller than the unstuffed scan");
    if (k + 1 < rows && m != (int32_t)(0xD0u + (k & 7u))) return jpeg_refuse("data ends early", "restart marker missing or out of order");
    segments[k].byte_offset = (uint32_t)start;
    segments[k].byte_count = (uint32_t)(used - start);
    segments[k].first_mcu = (uint32_t)(k * interval);
    segments[k].mcu_count = (uint32_t)(total - k * interval < interval ? total - k * interval : interval);
  }
  // what follows the scan: another scan or a DNL is refused, anything else (EOI, nothing) ends the image
  while (m >= 0xD0 && m <= 0xD7) m = s.next_marker();
  if (m == 0xDA) return jpeg_refuse("several scans");
  if (m == 0xDC) return jpeg_refuse("DNL segment");

  std::memset(tables, 0, sizeof(*tables));
  for (int c = 0; c < I.n_components; ++c) {
    copy_table(T.dc[I.comp[c].dc_table], &tables->dc[c]);
    copy_table(T.ac[I.comp[c].ac_table], &tables->ac[c]);
  }
  *scan_bytes = used;
  *n_segments = (uint32_t)rows;
  return ILCC_OK;
}

}  // extern "C"
