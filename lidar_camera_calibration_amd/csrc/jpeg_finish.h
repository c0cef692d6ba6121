// "K17's rows and scans of a batch -> each image's file", once for the chains that write JPEG files
// (jpeg_write_sequence_api.cpp, overlay_sequence_api.cpp).  Per batch: rows_back() queues the rows' copy behind K17; when the
// stream has been waited for, scans_back() checks the span and queues ONE copy of the scans that were produced; after the next wait
// file() hands out image i's file: headers + scan + EOI as three spans where K17 placed it (route 0), and else -- route 1, or
// an image without room in K17's output -- the host encoder's bytes of its coefficients (route 1).  The waits are the caller's, so
// that each chain keeps the copies and synchronisations it had.
//
// One pass in index order serves both callers: a fallback image's coefficients come back into a buffer of the finisher's own, not
// into the scan region of the pinned buffer, which still holds the scans of the images behind it.  (Sharing the region would save
// one page-locked allocation of an image's coefficients per finisher and cost a second pass: every route-0 file of a batch before
// its first fallback.)  Internal, not installed.
#pragma once

#include <string>
#include <vector>

#include "host_util.h"
#include "ilcc_jpeg_write.h"
#include "ilcc_jpeg_write_sequence.h"

namespace ilcc {

struct JpegFile {
  const uint8_t* part[3] = {nullptr, nullptr, nullptr};   // headers, scan, EOI; or the host encoder's file alone in part[0]
  uint64_t part_bytes[3] = {0, 0, 0};
  uint32_t route = 0;
  uint64_t bytes() const { return part_bytes[0] + part_bytes[1] + part_bytes[2]; }
};

struct JpegFinisher {
  // of a batch's images on the device; coefficients and scans with their pitches in bytes
  const ilcc_jpeg_info* info = nullptr;
  hipStream_t stream = nullptr;
  const uint8_t* d_coef = nullptr;
  uint64_t coef_pitch = 0;
  const uint8_t* d_scans = nullptr;
  const ilcc_jpeg_encode_row* d_rows = nullptr;
  uint64_t out_per_image = 0;
  uint8_t* h_back = nullptr;   // page-locked [ rows | scans ]: back_rows bytes, then out_per_image * the largest batch
  uint64_t back_rows = 0;
  // what it copied back and encoded so far
  uint64_t d2h_bytes = 0;
  int32_t n_host_encoded = 0;

  int32_t init();   // the headers, once, and the coefficient buffer
  int32_t rows_back(uint32_t n);
  int32_t scans_back(uint32_t n, bool* queued);
  // image i of the batch: route 0 asks for K17's scan and falls back, route 1 asks for the host encoder.  `encoded` takes the host
  // encoder's bytes; `name` ("message 12") starts the text of a failure.  The spans hold until the next scans_back().
  int32_t file(uint32_t i, uint32_t route, const std::string& name, std::vector<uint8_t>* encoded, JpegFile* f);

 private:
  uint8_t headers[1024];   // above the 629 bytes the headers can take
  uint64_t header_bytes = 0;
  Pinned h_coef;
};

}  // namespace ilcc
