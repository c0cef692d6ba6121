// The chained entries of include/ilcc_jpeg_write.h: pixels -> K14 (csrc/k14_jpeg_write.hip) -> the coefficients back to
// the host -> Huffman coding (csrc/jpeg_entropy_enc.cpp, host) -> the bytes of the file, from device pixels, from host
// pixels and from a bag's first frame (csrc/bag_frame.h).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>

#include "bag_frame.h"
#include "host_util.h"
#include "ilcc_hip.h"
#include "ilcc_jpeg_write.h"

using namespace ilcc;

namespace {

// where the parts of an encode lie behind `pixel_bytes` of pixels
JpegLayout encode_layout(const ilcc_jpeg_info& I, uint64_t pixel_bytes) { return JpegLayout(I, pixel_bytes, ilcc_jpeg_fdct_scratch_bytes(&I)); }

// K14 on `stream`, the coefficients to the host, the file into [out, out + cap)
int32_t encode_to(const ilcc_jpeg_info& I, const void* d_src, int32_t stride, int32_t encoding, void* d_coef, void* d_scratch,
                  uint64_t scratch_bytes, hipStream_t stream, uint8_t* out, uint64_t cap, uint64_t* bytes) {
  std::unique_ptr<int16_t[]> coef(new (std::nothrow) int16_t[I.coef_count]);
  if (!coef) return fail(ILCC_IO_ERROR, "out of memory for the JPEG's coefficients");
  const int32_t st = ilcc_jpeg_fdct_device(&I, d_src, stride, encoding, (int16_t*)d_coef, d_scratch, scratch_bytes, stream);
  if (st != ILCC_OK) return st;
  hipError_t e = hipMemcpyAsync(coef.get(), d_coef, I.coef_count * sizeof(int16_t), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hip_fail(e);
  return ilcc_jpeg_entropy_encode(&I, coef.get(), out, cap, bytes);
}

// the file in a buffer of this function's own: first one that holds any file an image compresses into, then the bound
int32_t encode_to_file(const ilcc_jpeg_info& I, const void* d_src, int32_t stride, int32_t encoding, void* d_coef, void* d_scratch,
                       uint64_t scratch_bytes, const char* path) {
  const uint64_t bound = ilcc_jpeg_file_bound(&I);
  uint64_t cap = 1024 + I.coef_count;   // a byte per coefficient: 8 bits a pixel
  for (;;) {
    if (cap > bound) cap = bound;
    std::unique_ptr<uint8_t[]> file(new (std::nothrow) uint8_t[cap]);
    if (!file) return fail(ILCC_IO_ERROR, "out of memory for the JPEG file");
    uint64_t bytes = 0;
    const int32_t st = encode_to(I, d_src, stride, encoding, d_coef, d_scratch, scratch_bytes, nullptr, file.get(), cap, &bytes);
    if (st == ILCC_CAPACITY && cap < bound) {
      cap = bound;
      continue;
    }
    if (st != ILCC_OK) return st;
    FILE* f = std::fopen(path, "wb");
    bool ok = f != nullptr;
    if (f) {
      ok = std::fwrite(file.get(), 1, bytes, f) == bytes;
      ok = (std::fclose(f) == 0) && ok;
    }
    return ok ? ILCC_OK : fail(ILCC_IO_ERROR, std::string("can not write ") + path);
  }
}

int32_t components_of(int32_t encoding) { return encoding == ILCC_ENCODING_MONO8 ? 1 : encoding == ILCC_ENCODING_BGR8 ? 3 : 0; }

// device bytes behind a mono8 image of this size for its coefficients (K14 needs no scratch for one component); 0 for a
// size the writer refuses
uint64_t mono8_encode_bytes(int32_t width, int32_t height) {
  ilcc_jpeg_info I;
  return ilcc_jpeg_write_info(width, height, 1, 1, 1, 95, 0, &I) == ILCC_OK ? encode_layout(I, 0).total : 0;
}

}  // namespace

extern "C" {

int32_t ilcc_jpeg_encode_device(const void* d_src, int32_t src_stride, int32_t width, int32_t height, int32_t encoding, int32_t quality,
                                int32_t sampling_h, int32_t sampling_v, int32_t restart_interval, uint8_t* out, uint64_t cap,
                                uint64_t* bytes, void* hip_stream) {
  if (!d_src || !bytes || (!out && cap)) return fail(ILCC_BAD_ARGUMENT, "ilcc_jpeg_encode_device: null argument");
  *bytes = 0;
  const int32_t nc = components_of(encoding);
  if (!nc) return fail(ILCC_BAD_ARGUMENT, "ilcc_jpeg_encode_device: mono8 or bgr8 pixels only");
  ilcc_jpeg_info I;
  int32_t st = ilcc_jpeg_write_info(width, height, nc, sampling_h, sampling_v, quality, restart_interval, &I);
  if (st != ILCC_OK) return st;
  if ((int64_t)src_stride < (int64_t)(nc == 1 ? 1 : 3) * width) return fail(ILCC_BAD_ARGUMENT, "ilcc_jpeg_encode_device: src_stride is shorter than a row");
  const JpegLayout E = encode_layout(I, 0);
  DeviceBuffer buf;
  const hipError_t e = hipMalloc(&buf.p, E.total);
  if (e != hipSuccess) return hip_fail(e);
  uint8_t* base = (uint8_t*)buf.p;
  st = encode_to(I, d_src, src_stride, encoding, base + E.coef_at, base + E.scratch_at, E.scratch_bytes, (hipStream_t)hip_stream, out, cap, bytes);
  if (st != ILCC_OK) (void)hipStreamSynchronize((hipStream_t)hip_stream);   // the buffer is freed on return
  return st;
}

int32_t ilcc_jpeg_write_file(int32_t device, const char* path, const uint8_t* pixels, int32_t stride, int32_t width, int32_t height,
                             int32_t encoding, int32_t quality) {
  if (!path || !pixels) return fail(ILCC_BAD_ARGUMENT, "ilcc_jpeg_write_file: null argument");
  const int32_t nc = components_of(encoding);
  if (!nc) return fail(ILCC_BAD_ARGUMENT, "ilcc_jpeg_write_file: mono8 or bgr8 pixels only");
  ilcc_jpeg_info I;
  int32_t st = ilcc_jpeg_write_info(width, height, nc, 2, 2, quality, 0, &I);   // 4:2:0: libjpeg's default
  if (st != ILCC_OK) return st;
  const uint64_t row = (uint64_t)(nc == 1 ? 1 : 3) * (uint64_t)width;
  if ((uint64_t)(stride < 0 ? 0 : stride) < row) return fail(ILCC_BAD_ARGUMENT, "ilcc_jpeg_write_file: stride is shorter than a row");
  st = select_device(device);
  if (st != ILCC_OK) return st;
  // ONE device buffer: [ pixels | coefficients | K14's scratch ]; the last row's padding is not read
  const uint64_t pixel_bytes = (uint64_t)(height - 1) * (uint64_t)stride + row;
  const JpegLayout E = encode_layout(I, pixel_bytes);
  DeviceBuffer buf;
  hipError_t e = hipMalloc(&buf.p, E.total);
  if (e == hipSuccess) e = hipMemcpy(buf.p, pixels, pixel_bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e);
  uint8_t* base = (uint8_t*)buf.p;
  return encode_to_file(I, base, stride, encoding, base + E.coef_at, base + E.scratch_at, E.scratch_bytes, path);
}

int32_t ilcc_bag_save_jpeg(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera,
                           const char* jpg_path, int32_t quality) {
  if (!jpg_path) return fail(ILCC_BAD_ARGUMENT, "ilcc_bag_save_jpeg: null argument");
  DeviceImage img;
  int32_t w = 0, h = 0;
  int32_t st = bag_image_to_device(device, bag_path, topic, camera, ~0ull, mono8_encode_bytes, &w, &h, &img);
  if (st != ILCC_OK) return st;
  ilcc_jpeg_info I;
  st = ilcc_jpeg_write_info(w, h, 1, 1, 1, quality, 0, &I);
  if (st != ILCC_OK) return st;
  if (!img.extra) return fail(ILCC_BAD_ARGUMENT, "ilcc_bag_save_jpeg: image larger than 65535 pixels a side");
  const JpegLayout E = encode_layout(I, 0);
  return encode_to_file(I, img.mono8, w, ILCC_ENCODING_MONO8, img.extra + E.coef_at, img.extra + E.scratch_at, E.scratch_bytes, jpg_path);
}

}  // extern "C"
