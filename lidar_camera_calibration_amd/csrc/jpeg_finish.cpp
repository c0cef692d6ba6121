// jpeg_finish.cpp -- K17's rows and scans of a batch into each image's file (jpeg_finish.h).  The headers and the host encoder are
// jpeg_entropy_enc.cpp's.  Failures are reported through ilcc_last_error(NULL).
#include "jpeg_finish.h"

#include <algorithm>

namespace ilcc {

namespace {
const uint8_t kEoi[2] = {0xFF, 0xD9};
}

int32_t JpegFinisher::init() {
  const hipError_t e = hipHostMalloc((void**)&h_coef.p, info->coef_count * sizeof(int16_t), hipHostMallocDefault);
  if (e != hipSuccess) return hip_fail(e);
  return ilcc_jpeg_write_headers(info, headers, sizeof(headers), &header_bytes);
}

int32_t JpegFinisher::rows_back(uint32_t n) {
  const hipError_t e = hipMemcpyAsync(h_back, d_rows, sizeof(ilcc_jpeg_encode_row) * n, hipMemcpyDeviceToHost, stream);
  if (e != hipSuccess) return hip_fail(e);
  d2h_bytes += sizeof(ilcc_jpeg_encode_row) * n;
  return ILCC_OK;
}

int32_t JpegFinisher::scans_back(uint32_t n, bool* queued) {
  const auto* rows = reinterpret_cast<const ilcc_jpeg_encode_row*>(h_back);
  uint64_t span = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (rows[i].status == 0) span = std::max(span, rows[i].offset + rows[i].bytes);
  if (span > out_per_image * n) return fail(ILCC_HIP_ERROR, "internal error: K17 placed a scan past its output");
  *queued = span != 0;
  if (!span) return ILCC_OK;
  const hipError_t e = hipMemcpyAsync(h_back + back_rows, d_scans, span, hipMemcpyDeviceToHost, stream);
  if (e != hipSuccess) return hip_fail(e);
  d2h_bytes += span;
  return ILCC_OK;
}

int32_t JpegFinisher::file(uint32_t i, uint32_t route, const std::string& name, std::vector<uint8_t>* encoded, JpegFile* f) {
  const ilcc_jpeg_encode_row* row = route == 0 ? reinterpret_cast<const ilcc_jpeg_encode_row*>(h_back) + i : nullptr;
  *f = JpegFile{};
  if (row && row->status == 0) {   // headers + scan + EOI
    f->part[0] = headers;
    f->part_bytes[0] = header_bytes;
    f->part[1] = h_back + back_rows + row->offset;
    f->part_bytes[1] = row->bytes;
    f->part[2] = kEoi;
    f->part_bytes[2] = 2;
    return ILCC_OK;
  }
  // route 1, or what K17 did not place: an image without room is finished by the host encoder; a range refusal is its to word
  const uint64_t coef_bytes = info->coef_count * sizeof(int16_t);
  hipError_t e = hipMemcpyAsync(h_coef.p, d_coef + coef_pitch * i, coef_bytes, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hip_fail(e);
  d2h_bytes += coef_bytes;
  const uint64_t bound = ilcc_jpeg_file_bound(info);
  uint64_t room = std::min<uint64_t>(1024 + info->coef_count, bound), n = 0;   // a byte per coefficient holds any file an image compresses into
  for (;;) {
    encoded->resize(room);
    const int32_t s = ilcc_jpeg_entropy_encode(info, reinterpret_cast<const int16_t*>(h_coef.p), encoded->data(), room, &n);
    if (s == ILCC_CAPACITY && room < bound) {
      room = bound;
      continue;
    }
    if (s != ILCC_OK) return fail(s, name + ": " + ilcc_last_error(nullptr));
    break;
  }
  encoded->resize(n);
  ++n_host_encoded;
  f->part[0] = encoded->data();
  f->part_bytes[0] = n;
  f->route = 1;
  if (row && (row->status & (ILCC_JPEG_ENCODE_DC_RANGE | ILCC_JPEG_ENCODE_AC_RANGE)))
    return fail(ILCC_HIP_ERROR, name + ": internal error: K17 refused coefficients (status " + std::to_string(row->status) + ") that the host encoder accepts");
  return ILCC_OK;
}

}  // namespace ilcc
