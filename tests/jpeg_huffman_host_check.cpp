// Stand-alone check of csrc/jpeg_scan_prepare.cpp, built by tests/test_jpeg_huffman_cpu.py with -fsanitize=address,undefined and
// linked with that file and csrc/jpeg_entropy.cpp only:
//
//   jpeg_huffman_host_check intact.jpg ... -- with_an_empty_segment.jpg ...
//
// Every file in front of "--" is prepared whole (ILCC_OK; with a scan buffer or a segment table one short: ILCC_CAPACITY) and then as
// each of its prefixes: every call returns ILCC_OK or ILCC_BAD_ARGUMENT, what prepare refuses the host decoder refuses too, and the
// rows of an accepted input tile the unstuffed scan and the image's MCUs.  Every file behind "--" must be accepted with at least one
// row of 0 bytes (which the host decoder refuses: K16 reports it).  The input, the scan buffer and the segment table each sit in a
// heap block of exactly the size handed over, so a read or write past it is a sanitizer report.  Exit status 0: all held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ilcc_hip.h"
#include "ilcc_jpeg.h"
#include "ilcc_jpeg_huffman.h"

namespace {

std::vector<uint8_t> file_bytes(const char* path) {
  std::vector<uint8_t> out;
  FILE* f = std::fopen(path, "rb");
  if (!f) return out;
  uint8_t buf[4096];
  for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) out.insert(out.end(), buf, buf + n);
  std::fclose(f);
  return out;
}

struct Prepared {
  int32_t status = ILCC_OK;      // of parse, bound or prepare: the step that ended it
  bool parsed = false;
  int32_t host = ILCC_OK;        // ilcc_jpeg_entropy_decode on the same bytes
  uint64_t scan_bytes = 0, bound_bytes = 0;
  uint32_t n_rows = 0, bound_rows = 0, empty_rows = 0;
  bool rows_tile = true;
};

// parse + bound + prepare of exactly `n` bytes, with `short_scan` / `short_rows` taken off the bound's capacities when the file's
// own sizes are known (exact_* != 0: capacity = exact - short)
Prepared prepare(const uint8_t* data, size_t n, uint64_t exact_scan = 0, uint32_t exact_rows = 0, uint32_t short_scan = 0, uint32_t short_rows = 0) {
  Prepared p;
  uint8_t* exact = (uint8_t*)std::malloc(n ? n : 1);
  if (n) std::memcpy(exact, data, n);
  ilcc_jpeg_info info;
  p.status = ilcc_jpeg_parse(exact, n, &info);
  if (p.status == ILCC_OK && info.coef_count <= (64u << 20)) {
    p.parsed = true;
    p.status = ilcc_jpeg_scan_bound(&info, n, &p.bound_bytes, &p.bound_rows);
    if (p.status == ILCC_OK) {
      const uint64_t scan_cap = exact_scan || short_scan ? exact_scan - short_scan : p.bound_bytes;
      const uint32_t row_cap = exact_rows || short_rows ? exact_rows - short_rows : p.bound_rows;
      uint8_t* scan = (uint8_t*)std::malloc(scan_cap ? scan_cap : 1);
      ilcc_jpeg_huffman_segment* rows = (ilcc_jpeg_huffman_segment*)std::malloc(row_cap ? row_cap * sizeof(ilcc_jpeg_huffman_segment) : 1);
      ilcc_jpeg_huffman_tables* tables = (ilcc_jpeg_huffman_tables*)std::malloc(sizeof(ilcc_jpeg_huffman_tables));
      p.status = ilcc_jpeg_scan_prepare(exact, n, &info, scan_cap ? scan : nullptr, scan_cap, &p.scan_bytes, row_cap ? rows : nullptr, row_cap,
                                        &p.n_rows, tables);
      if (p.status == ILCC_OK) {
        const uint64_t mcus = (uint64_t)(info.comp[0].blocks_w / info.comp[0].h) * (uint64_t)(info.comp[0].blocks_h / info.comp[0].v);
        uint64_t at = 0, mcu = 0;
        for (uint32_t k = 0; k < p.n_rows; ++k) {
          if (rows[k].byte_offset != at || rows[k].first_mcu != mcu || rows[k].mcu_count == 0) p.rows_tile = false;
          at += rows[k].byte_count;
          mcu += rows[k].mcu_count;
          if (rows[k].byte_count == 0) ++p.empty_rows;
        }
        if (at != p.scan_bytes || mcu != mcus || p.scan_bytes > p.bound_bytes || p.n_rows != p.bound_rows) p.rows_tile = false;
        for (int c = info.n_components; c < 3; ++c)
          for (size_t b = 0; b < sizeof(ilcc_jpeg_huffman_table); ++b)
            if (((const uint8_t*)&tables->dc[c])[b] || ((const uint8_t*)&tables->ac[c])[b]) p.rows_tile = false;
      }
      std::free(tables);
      std::free(rows);
      std::free(scan);
    }
    int16_t* coef = (int16_t*)std::malloc(info.coef_count * sizeof(int16_t) + 2);
    p.host = ilcc_jpeg_entropy_decode(exact, n, &info, coef, info.coef_count);
    std::free(coef);
  }
  std::free(exact);
  return p;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  long calls = 0;
  int at = 1;
  for (; at < argc && std::strcmp(argv[at], "--") != 0; ++at) {
    const std::vector<uint8_t> jpg = file_bytes(argv[at]);
    if (jpg.empty()) return 2;
    const Prepared whole = prepare(jpg.data(), jpg.size());
    if (whole.status != ILCC_OK || !whole.rows_tile || whole.host != ILCC_OK) {
      std::fprintf(stderr, "%s: status %d, rows tile %d, host %d\n", argv[at], whole.status, (int)whole.rows_tile, whole.host);
      return 1;
    }
    const Prepared exact = prepare(jpg.data(), jpg.size(), whole.scan_bytes, whole.n_rows);
    const Prepared short_scan = prepare(jpg.data(), jpg.size(), whole.scan_bytes, whole.n_rows, 1, 0);
    const Prepared short_rows = prepare(jpg.data(), jpg.size(), whole.scan_bytes, whole.n_rows, 0, 1);
    if (exact.status != ILCC_OK || short_scan.status != ILCC_CAPACITY || short_rows.status != ILCC_CAPACITY) {
      std::fprintf(stderr, "%s: capacities exact / one byte short / one row short: status %d / %d / %d\n", argv[at], exact.status,
                   short_scan.status, short_rows.status);
      return 1;
    }
    for (size_t n = 0; n < jpg.size(); ++n, ++calls) {
      const Prepared p = prepare(jpg.data(), n);
      const bool status_ok = p.status == ILCC_OK || p.status == ILCC_BAD_ARGUMENT;
      const bool host_agrees = !p.parsed || p.status == ILCC_OK || p.host != ILCC_OK;   // what prepare refuses, the decoder refuses
      if (!status_ok || !host_agrees || (p.status == ILCC_OK && p.parsed && !p.rows_tile)) {
        std::fprintf(stderr, "%s: prefix %zu: status %d, host %d, rows tile %d\n", argv[at], n, p.status, p.host, (int)p.rows_tile);
        return 1;
      }
    }
  }
  long empties = 0;
  for (++at; at < argc; ++at) {
    const std::vector<uint8_t> jpg = file_bytes(argv[at]);
    if (jpg.empty()) return 2;
    const Prepared p = prepare(jpg.data(), jpg.size());
    if (p.status != ILCC_OK || !p.rows_tile || p.empty_rows == 0 || p.host != ILCC_BAD_ARGUMENT) {
      std::fprintf(stderr, "%s: status %d, rows tile %d, empty rows %u, host %d\n", argv[at], p.status, (int)p.rows_tile, p.empty_rows, p.host);
      return 1;
    }
    empties += p.empty_rows;
  }
  std::printf("%ld prefixes: every status ILCC_OK or ILCC_BAD_ARGUMENT; %ld empty segments accepted\n", calls, empties);
  return 0;
}
