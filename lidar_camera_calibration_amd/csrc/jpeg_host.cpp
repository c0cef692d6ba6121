// The chained entries of include/ilcc_jpeg.h: file or message -> parse -> entropy decode (csrc/jpeg_entropy.cpp, host) ->
// upload -> K13 (csrc/k13_jpeg.hip), the sensor_msgs/CompressedImage parser, and the helper through which the bag entries
// take the first frame of a camera topic whichever of the two message types carries it (csrc/bag_frame.h).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "bag_frame.h"
#include "host_util.h"
#include "ilcc_hip.h"
#include "ilcc_image_corners.h"
#include "ilcc_ingest.h"
#include "ilcc_jpeg.h"
#include "jpeg_entropy.h"

using namespace ilcc;

namespace {


// the refusals of jpeg_entropy.cpp, which knows nothing of the library, arrive in ilcc_last_error
const bool g_sink_set = (jpeg_error_sink = [](const char* text) { set_global_error(text); }, true);

int bytes_per_pixel(const ilcc_jpeg_info& I) { return I.n_components == 1 ? 1 : 3; }

// where the parts of a decode lie behind `pixel_bytes` of pixels
JpegLayout decode_layout(const ilcc_jpeg_info& I, uint64_t pixel_bytes) { return JpegLayout(I, pixel_bytes, ilcc_jpeg_scratch_bytes(&I)); }

// entropy decode on the host, coefficients to d_coef, K13 into d_pixels on `stream`
int32_t decode_to(const uint8_t* jpg, uint64_t bytes, const ilcc_jpeg_info& I, void* d_pixels, int32_t stride, void* d_coef, void* d_scratch,
                  uint64_t scratch_bytes, hipStream_t stream) {
  std::vector<int16_t> coef;
  try {
    coef.resize(I.coef_count);
  } catch (...) {   // no exception crosses the C-ABI
    return fail(ILCC_IO_ERROR, "out of memory for the JPEG's coefficients");
  }
  const int32_t st = ilcc_jpeg_entropy_decode(jpg, bytes, &I, coef.data(), coef.size());
  if (st != ILCC_OK) return st;
  const hipError_t e = hipMemcpy(d_coef, coef.data(), coef.size() * sizeof(int16_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e);
  return ilcc_jpeg_idct_device(&I, (const int16_t*)d_coef, d_pixels, stride, d_scratch, scratch_bytes, stream);
}

bool contains(const uint8_t* text, uint32_t len, const char* word) {
  const size_t w = std::strlen(word);
  for (uint32_t i = 0; i + w <= len; ++i)
    if (std::memcmp(text + i, word, w) == 0) return true;
  return false;
}

}  // namespace

namespace ilcc {

int32_t bag_frame_read(const char* bag_path, const char* topic, BagFrame* out) {
  int32_t st = read_first_message(bag_path, topic, kImageMd5, &out->msg);
  if (st == ILCC_OK) {
    out->compressed = false;
    st = ilcc_image_parse_any(out->msg.data(), out->msg.size(), &out->L);   // Bayer topics too: K11 demosaics them
    if (st != ILCC_OK) return st;
    out->device_bytes = (uint64_t)out->L.step * out->L.height;   // <= data_bytes (ilcc_image_parse_any)
    return ILCC_OK;
  }
  if (st != ILCC_BAD_ARGUMENT) return st;
  // no sensor_msgs/Image there (or an argument both reads refuse alike): the topic's first CompressedImage
  st = read_first_message(bag_path, topic, kCompressedImageMd5, &out->msg);
  if (st != ILCC_OK) return st;
  ilcc_compressed_image_layout C;
  st = ilcc_compressed_image_parse(out->msg.data(), out->msg.size(), &C);
  if (st != ILCC_OK) return st;
  st = ilcc_jpeg_parse(out->msg.data() + C.data_offset, C.data_bytes, &out->jpeg);
  if (st != ILCC_OK) return st;
  out->compressed = true;
  ilcc_image_layout& L = out->L;
  std::memset(&L, 0, sizeof(L));
  L.width = (uint32_t)out->jpeg.width;
  L.height = (uint32_t)out->jpeg.height;
  L.step = (uint32_t)(bytes_per_pixel(out->jpeg) * out->jpeg.width);
  L.encoding = out->jpeg.n_components == 1 ? ILCC_ENCODING_MONO8 : ILCC_ENCODING_BGR8;
  L.stamp_sec = C.stamp_sec;
  L.stamp_nsec = C.stamp_nsec;
  L.seq = C.seq;
  L.data_offset = C.data_offset;
  L.data_bytes = C.data_bytes;
  std::memcpy(L.frame_id, C.frame_id, sizeof(L.frame_id));
  out->device_bytes = decode_layout(out->jpeg, (uint64_t)L.step * L.height).total;
  return ILCC_OK;
}

int32_t bag_frame_to_device(const BagFrame& f, void* d_mem) {
  const uint8_t* data = f.msg.data() + f.L.data_offset;
  if (!f.compressed) {
    const hipError_t e = hipMemcpy(d_mem, data, (uint64_t)f.L.step * f.L.height, hipMemcpyHostToDevice);
    return e == hipSuccess ? ILCC_OK : hip_fail(e);
  }
  const JpegLayout D = decode_layout(f.jpeg, (uint64_t)f.L.step * f.L.height);
  uint8_t* base = (uint8_t*)d_mem;
  return decode_to(data, f.L.data_bytes, f.jpeg, base, (int32_t)f.L.step, base + D.coef_at, base + D.scratch_at, D.scratch_bytes, nullptr);
}

}  // namespace ilcc

extern "C" {

int32_t ilcc_jpeg_decode_device(const uint8_t* jpg, uint64_t bytes, void* d_dst, int32_t dst_stride, uint64_t cap_bytes, int32_t* width,
                                int32_t* height, int32_t* encoding, void* hip_stream) {
  if (!jpg || !width || !height || !encoding || (!d_dst && cap_bytes)) return fail(ILCC_BAD_ARGUMENT, "ilcc_jpeg_decode_device: null argument");
  *width = *height = *encoding = 0;
  ilcc_jpeg_info I;
  int32_t st = ilcc_jpeg_parse(jpg, bytes, &I);
  if (st != ILCC_OK) return st;
  const int bpp = bytes_per_pixel(I);
  *width = I.width;
  *height = I.height;
  *encoding = bpp == 1 ? ILCC_ENCODING_MONO8 : ILCC_ENCODING_BGR8;
  if ((int64_t)dst_stride < (int64_t)bpp * I.width) return fail(ILCC_BAD_ARGUMENT, "ilcc_jpeg_decode_device: dst_stride is shorter than a row");
  if (cap_bytes < (uint64_t)(I.height - 1) * (uint64_t)dst_stride + (uint64_t)bpp * (uint64_t)I.width)
    return fail(ILCC_CAPACITY, "image larger than the buffer");
  const JpegLayout D = decode_layout(I, 0);
  DeviceBuffer buf;
  const hipError_t e = hipMalloc(&buf.p, D.total);
  if (e != hipSuccess) return hip_fail(e);
  uint8_t* base = (uint8_t*)buf.p;
  st = decode_to(jpg, bytes, I, d_dst, dst_stride, base + D.coef_at, base + D.scratch_at, D.scratch_bytes, (hipStream_t)hip_stream);
  const hipError_t done = hipStreamSynchronize((hipStream_t)hip_stream);   // the buffer is freed on return
  if (st == ILCC_OK && done != hipSuccess) return hip_fail(done);
  return st;
}

int32_t ilcc_jpeg_find_chessboard(int32_t device, const char* jpg_path, const ilcc_camera_model* camera, int32_t board_w, int32_t board_h,
                                  int32_t* rows, int32_t* cols, double* xy) {
  if (!jpg_path || !rows || !cols || !xy || board_w < 3 || board_h < 3) return fail(ILCC_BAD_ARGUMENT, "ilcc_jpeg_find_chessboard: bad argument");
  *rows = *cols = 0;
  std::vector<uint8_t> jpg;
  try {
    std::ifstream in(jpg_path, std::ios::binary);
    if (!in.is_open()) return fail(ILCC_IO_ERROR, std::string("can not open ") + jpg_path);
    jpg.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
  } catch (...) {   // no exception crosses the C-ABI
    return fail(ILCC_IO_ERROR, std::string("cannot read ") + jpg_path);
  }
  ilcc_jpeg_info I;
  int32_t st = ilcc_jpeg_parse(jpg.data(), jpg.size(), &I);
  if (st != ILCC_OK) return st;
  if (camera && (camera->width != I.width || camera->height != I.height))
    return fail(ILCC_BAD_ARGUMENT, "the camera's width / height differ from the image's");
  st = select_device(device);
  if (st != ILCC_OK) return st;
  // ONE device buffer: [ the file's pixels | coefficients | K13's scratch | mono8 ]
  const int32_t step = bytes_per_pixel(I) * I.width;
  const JpegLayout D = decode_layout(I, (uint64_t)step * (uint64_t)I.height);
  DeviceBuffer buf;
  const hipError_t e = hipMalloc(&buf.p, D.total + (uint64_t)I.width * (uint64_t)I.height);
  if (e != hipSuccess) return hip_fail(e);
  uint8_t* base = (uint8_t*)buf.p;
  uint8_t* mono8 = base + D.total;
  st = decode_to(jpg.data(), jpg.size(), I, base, step, base + D.coef_at, base + D.scratch_at, D.scratch_bytes, nullptr);
  if (st != ILCC_OK) return st;
  st = ilcc_image_to_mono8_device(base, I.width, I.height, step, I.n_components == 1 ? ILCC_ENCODING_MONO8 : ILCC_ENCODING_BGR8, camera,
                                  mono8, I.width, nullptr);
  if (st != ILCC_OK) return st;
  return ilcc_find_chessboard_device(mono8, I.width, I.height, I.width, board_w, board_h, rows, cols, xy, nullptr);   // the same (default) stream
}

int32_t ilcc_compressed_image_parse(const uint8_t* m, uint64_t n, ilcc_compressed_image_layout* out) {
  if (!m || !out) return fail(ILCC_BAD_ARGUMENT, "ilcc_compressed_image_parse: null argument");
  std::memset(out, 0, sizeof(*out));
  const char* truncated = "CompressedImage message truncated";
  uint64_t at = 0;
  uint32_t len = 0;
  if (!read_header(m, n, &at, &out->seq, &out->stamp_sec, &out->stamp_nsec, out->frame_id)) return fail(ILCC_BAD_ARGUMENT, truncated);
  if (!read_u32(m, n, &at, &len) || len > n - at) return fail(ILCC_BAD_ARGUMENT, truncated);
  const uint8_t* format = m + at;
  const uint32_t format_len = len;
  std::memcpy(out->format, m + at, len < sizeof(out->format) - 1 ? len : sizeof(out->format) - 1);
  at += len;
  uint32_t data_len = 0;
  if (!read_u32(m, n, &at, &data_len)) return fail(ILCC_BAD_ARGUMENT, truncated);
  out->data_offset = at;
  out->data_bytes = data_len;
  if (data_len > n - at) return fail(ILCC_BAD_ARGUMENT, "CompressedImage data[] length runs past the message");
  if (!contains(format, format_len, "jpeg") && !contains(format, format_len, "jpg")) {
    char text[128];
    std::snprintf(text, sizeof(text), "unsupported CompressedImage format '%.40s' (only jpeg)", out->format);
    return fail(ILCC_BAD_ARGUMENT, text);
  }
  if (data_len == 0) return fail(ILCC_BAD_ARGUMENT, "empty CompressedImage");
  return ILCC_OK;
}

}  // extern "C"
