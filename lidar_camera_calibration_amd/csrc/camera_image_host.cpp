// Host side of include/ilcc_camera_image.h: the intrinsics reader (what ImageCornersEst::getRectifyParam,
// /root/reference/ilcc2/src/ImageCornersEst.cpp:15-61, takes from cv::FileStorage), the sensor_msgs/Image
// parser, and the two bag entries that chain the topic's first frame (csrc/bag_frame.h) -> K11
// (/root/reference/ilcc2/test/get_image_corners_bag.cpp:67-112).  Little-endian host.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "bag_frame.h"
#include "host_util.h"
#include "ilcc_camera_image.h"
#include "ilcc_hip.h"
#include "ilcc_image_corners.h"
#include "ilcc_ingest.h"

using namespace ilcc;

namespace {

std::string trimmed(const std::string& s) {
  const size_t a = s.find_first_not_of(" \t\r\n");
  const size_t b = s.find_last_not_of(" \t\r\n");
  return a == std::string::npos ? std::string() : s.substr(a, b - a + 1);
}

struct Matrix {
  long rows = -1, cols = -1;
  std::string dt;
  std::vector<double> data;
};

// every number of "a, b, c" -> out; false on anything that is not a number
bool parse_numbers(const std::string& list, std::vector<double>* out) {
  std::stringstream ss(list);
  std::string item;
  while (std::getline(ss, item, ',')) {
    item = trimmed(item);
    if (item.empty()) continue;   // a trailing comma before a line break
    char* end = nullptr;
    const double v = std::strtod(item.c_str(), &end);
    if (end == item.c_str() || *end != '\0') return false;
    out->push_back(v);
  }
  return true;
}

// The lines of an OpenCV-FileStorage YAML (comments stripped).  `name: !!opencv-matrix` opens a block of indented
// `rows:` / `cols:` / `dt:` / `data: [ ... ]` lines (data may run over several lines); anything else is `key: scalar`.
struct Yaml {
  std::vector<std::string> lines;

  bool scalar(const std::string& key, double* v) const {
    for (const std::string& l : lines) {
      const size_t colon = l.find(':');
      if (colon == std::string::npos || trimmed(l.substr(0, colon)) != key || l[0] == ' ' || l[0] == '\t') continue;
      const std::string val = trimmed(l.substr(colon + 1));
      char* end = nullptr;
      *v = std::strtod(val.c_str(), &end);
      return end != val.c_str() && *end == '\0';
    }
    return false;
  }

  // 0: no such block; 1: read; -1: malformed
  int matrix(const std::string& name, Matrix* m) const {
    size_t at = 0;
    for (; at < lines.size(); ++at) {
      const std::string& l = lines[at];
      const size_t colon = l.find(':');
      if (colon == std::string::npos || l[0] == ' ' || l[0] == '\t' || trimmed(l.substr(0, colon)) != name) continue;
      if (trimmed(l.substr(colon + 1)) != "!!opencv-matrix") return -1;
      break;
    }
    if (at == lines.size()) return 0;
    bool have_data = false;
    for (++at; at < lines.size(); ++at) {
      const std::string& l = lines[at];
      if (l[0] != ' ' && l[0] != '\t') break;   // the block ends at the next top-level key
      const size_t colon = l.find(':');
      if (colon == std::string::npos) return -1;
      const std::string key = trimmed(l.substr(0, colon));
      std::string val = trimmed(l.substr(colon + 1));
      if (key == "rows" || key == "cols") {
        char* end = nullptr;
        const long v = std::strtol(val.c_str(), &end, 10);
        if (end == val.c_str() || *end != '\0') return -1;
        (key == "rows" ? m->rows : m->cols) = v;
      } else if (key == "dt") {
        m->dt = val;
      } else if (key == "data") {
        while (val.find(']') == std::string::npos && at + 1 < lines.size()) val += " " + trimmed(lines[++at]);
        const size_t open = val.find('['), close = val.find(']');
        if (open == std::string::npos || close == std::string::npos || close < open) return -1;
        if (!parse_numbers(val.substr(open + 1, close - open - 1), &m->data)) return -1;
        have_data = true;
      }
    }
    return have_data ? 1 : -1;
  }
};

// every encoding name a layout can carry; `wide`: taken by ilcc_image_parse_any only (callers of ilcc_image_parse index
// the first five with layout.encoding)
const struct {
  const char* name;
  uint32_t encoding, bpp;
  bool wide;
} kKnownEncodings[] = {{"mono8", ILCC_ENCODING_MONO8, 1, false},
                       {"bgr8", ILCC_ENCODING_BGR8, 3, false},
                       {"rgb8", ILCC_ENCODING_RGB8, 3, false},
                       {"bgra8", ILCC_ENCODING_BGRA8, 4, false},
                       {"rgba8", ILCC_ENCODING_RGBA8, 4, false},
                       {"bayer_rggb8", ILCC_ENCODING_BAYER_RGGB8, 1, true},
                       {"bayer_bggr8", ILCC_ENCODING_BAYER_BGGR8, 1, true},
                       {"bayer_gbrg8", ILCC_ENCODING_BAYER_GBRG8, 1, true},
                       {"bayer_grbg8", ILCC_ENCODING_BAYER_GRBG8, 1, true}};

// ilcc_image_parse (wide = false) and ilcc_image_parse_any (wide = true)
int32_t parse_image(const uint8_t* m, uint64_t n, ilcc_image_layout* out, bool wide) {
  if (!m || !out) return fail(ILCC_BAD_ARGUMENT, wide ? "ilcc_image_parse_any: null argument" : "ilcc_image_parse: null argument");
  std::memset(out, 0, sizeof(*out));
  const char* truncated = "Image message truncated";
  uint64_t at = 0;
  uint32_t len = 0;
  if (!read_header(m, n, &at, &out->seq, &out->stamp_sec, &out->stamp_nsec, out->frame_id)) return fail(ILCC_BAD_ARGUMENT, truncated);
  if (!read_u32(m, n, &at, &out->height) || !read_u32(m, n, &at, &out->width) || !read_u32(m, n, &at, &len) || len > n - at)
    return fail(ILCC_BAD_ARGUMENT, truncated);
  const char* enc = (const char*)m + at;
  const uint32_t enc_len = len;
  at += len;
  uint32_t data_len = 0;
  if (n - at < 1) return fail(ILCC_BAD_ARGUMENT, truncated);
  out->is_bigendian = m[at++];
  if (!read_u32(m, n, &at, &out->step) || !read_u32(m, n, &at, &data_len)) return fail(ILCC_BAD_ARGUMENT, truncated);
  out->data_offset = at;
  out->data_bytes = data_len;
  if (data_len > n - at) return fail(ILCC_BAD_ARGUMENT, "Image data[] length runs past the message");
  uint32_t bpp = 0;
  bool bayer = false;
  for (const auto& k : kKnownEncodings)
    if ((wide || !k.wide) && std::strlen(k.name) == enc_len && std::memcmp(k.name, enc, enc_len) == 0) {
      out->encoding = k.encoding;
      bpp = k.bpp;
      bayer = k.wide;
    }
  if (!bpp) {
    char text[96];
    std::snprintf(text, sizeof(text), "unsupported Image encoding '%.*s'", (int)(enc_len < 40 ? enc_len : 40), enc);
    return fail(ILCC_BAD_ARGUMENT, text);
  }
  if (out->width == 0 || out->height == 0) return fail(ILCC_BAD_ARGUMENT, "empty Image");
  if (bayer && (out->width < 3 || out->height < 3)) return fail(ILCC_BAD_ARGUMENT, "a Bayer Image must be at least 3 x 3");
  if ((uint64_t)out->step < (uint64_t)out->width * bpp) return fail(ILCC_BAD_ARGUMENT, "Image step is shorter than a row");
  if (out->data_bytes < (uint64_t)out->step * out->height) return fail(ILCC_BAD_ARGUMENT, "Image data[] is shorter than step * height");
  return ILCC_OK;
}

}  // namespace

int32_t ilcc::bag_image_to_device(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera,
                                  uint64_t cap_pixels, uint64_t (*extra_for)(int32_t, int32_t), int32_t* width, int32_t* height,
                                  DeviceImage* out) {
  BagFrame frame;
  int32_t st = bag_frame_read(bag_path, topic, &frame);
  if (st != ILCC_OK) return st;
  ilcc_image_layout& L = out->L;
  L = frame.L;
  if (L.width > 65536u || L.height > 65536u) return fail(ILCC_BAD_ARGUMENT, "image larger than 65536 pixels a side");
  *width = (int32_t)L.width;
  *height = (int32_t)L.height;
  const uint64_t pixels = (uint64_t)L.width * L.height;
  if (pixels > cap_pixels) return fail(ILCC_CAPACITY, "image larger than the buffer");
  if (camera && (camera->width != *width || camera->height != *height))
    return fail(ILCC_BAD_ARGUMENT, "the camera's width / height differ from the image's");
  if (L.step > (uint32_t)INT32_MAX) return fail(ILCC_BAD_ARGUMENT, "image step too large");
  st = select_device(device);
  if (st != ILCC_OK) return st;
  const uint64_t mono_at = align256(frame.device_bytes);
  const uint64_t extra_at = align256(mono_at + pixels);
  const uint64_t extra_bytes = extra_for ? extra_for(*width, *height) : 0;
  const hipError_t e = hipMalloc(&out->buffer.p, extra_bytes ? extra_at + extra_bytes : mono_at + pixels);
  if (e != hipSuccess) return hip_fail(e);
  uint8_t* base = (uint8_t*)out->buffer.p;
  st = bag_frame_to_device(frame, base);
  if (st != ILCC_OK) return st;
  out->mono8 = base + mono_at;
  out->extra = extra_bytes ? base + extra_at : nullptr;
  return ilcc_image_to_mono8_device(base, *width, *height, (int32_t)L.step, (int32_t)L.encoding, camera, out->mono8, *width,
                                    nullptr);
}

extern "C" {

int32_t ilcc_read_camera_yaml(const char* path, ilcc_camera_model* out) {
  if (!path || !out) return fail(ILCC_BAD_ARGUMENT, "ilcc_read_camera_yaml: null argument");
  try {
    std::ifstream in(path);
    if (!in.is_open()) return fail(ILCC_IO_ERROR, std::string("can not open ") + path);
    Yaml y;
    std::string line;
    while (std::getline(in, line)) {
      const size_t hash = line.find('#');
      if (hash != std::string::npos) line.erase(hash);
      if (!trimmed(line).empty()) y.lines.push_back(line);
    }
    Matrix K, d;
    int got = y.matrix("K", &K);
    if (got == 0) return fail(ILCC_BAD_ARGUMENT, std::string("no matrix K in ") + path);
    if (got < 0 || K.rows != 3 || K.cols != 3 || K.dt != "d" || K.data.size() != 9)
      return fail(ILCC_BAD_ARGUMENT, "K must be a 3 x 3 !!opencv-matrix of dt: d");
    got = y.matrix("d", &d);
    if (got == 0) return fail(ILCC_BAD_ARGUMENT, std::string("no matrix d in ") + path);
    const bool vec = (d.rows == 1 || d.cols == 1) && d.rows * d.cols == (long)d.data.size();
    if (got < 0 || !vec || d.dt != "d" || (d.data.size() != 4 && d.data.size() != 5))
      return fail(ILCC_BAD_ARGUMENT, "d must be a !!opencv-matrix of dt: d with 4 or 5 entries in one row or column");
    if (K.data[1] != 0) return fail(ILCC_BAD_ARGUMENT, "K has non-zero skew: not supported");
    if (K.data[3] != 0 || K.data[6] != 0 || K.data[7] != 0 || K.data[8] != 1)
      return fail(ILCC_BAD_ARGUMENT, "K is not a camera matrix: its last row must be (0, 0, 1)");
    for (double v : K.data)
      if (!std::isfinite(v)) return fail(ILCC_BAD_ARGUMENT, "K holds a non-finite entry");
    for (double v : d.data)
      if (!std::isfinite(v)) return fail(ILCC_BAD_ARGUMENT, "d holds a non-finite entry");
    if (K.data[0] == 0 || K.data[4] == 0) return fail(ILCC_BAD_ARGUMENT, "fx and fy must be non-zero");
    double w = 0, h = 0;
    if (!y.scalar("Camera.width", &w) || !y.scalar("Camera.height", &h) || !(w >= 1) || !(h >= 1) || w > 65536 || h > 65536 ||
        w != std::floor(w) || h != std::floor(h))
      return fail(ILCC_BAD_ARGUMENT, "Camera.width / Camera.height missing or invalid");
    std::memset(out, 0, sizeof(*out));
    out->fx = K.data[0];
    out->cx = K.data[2];
    out->fy = K.data[4];
    out->cy = K.data[5];
    for (size_t k = 0; k < d.data.size(); ++k) out->d[k] = d.data[k];   // a missing k3 stays 0
    out->width = (int32_t)w;
    out->height = (int32_t)h;
    return ILCC_OK;
  } catch (...) {   // no exception crosses the C-ABI
    return fail(ILCC_IO_ERROR, std::string("cannot read ") + path);
  }
}

int32_t ilcc_image_parse(const uint8_t* m, uint64_t n, ilcc_image_layout* out) { return parse_image(m, n, out, false); }

int32_t ilcc_image_parse_any(const uint8_t* m, uint64_t n, ilcc_image_layout* out) { return parse_image(m, n, out, true); }

int32_t ilcc_bag_first_image(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera,
                             uint8_t* mono8_out, uint64_t cap_bytes, int32_t* width, int32_t* height) {
  if (!width || !height || (!mono8_out && cap_bytes)) return fail(ILCC_BAD_ARGUMENT, "ilcc_bag_first_image: null argument");
  *width = *height = 0;
  DeviceImage img;
  const int32_t st = bag_image_to_device(device, bag_path, topic, camera, cap_bytes, nullptr, width, height, &img);
  if (st != ILCC_OK) return st;
  const hipError_t e = hipMemcpy(mono8_out, img.mono8, (size_t)*width * (size_t)*height, hipMemcpyDeviceToHost);   // waits for K11
  if (e != hipSuccess) return hip_fail(e);
  return ILCC_OK;
}

int32_t ilcc_bag_find_chessboard(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera,
                                 int32_t board_w, int32_t board_h, int32_t* rows, int32_t* cols, double* xy) {
  if (!rows || !cols || !xy || board_w < 3 || board_h < 3) return fail(ILCC_BAD_ARGUMENT, "ilcc_bag_find_chessboard: bad argument");
  *rows = *cols = 0;
  DeviceImage img;
  int32_t w = 0, h = 0;
  const int32_t st = bag_image_to_device(device, bag_path, topic, camera, ~0ull, nullptr, &w, &h, &img);
  if (st != ILCC_OK) return st;
  return ilcc_find_chessboard_device(img.mono8, w, h, w, board_w, board_h, rows, cols, xy, nullptr);   // the same (default) stream as K11
}

}  // extern "C"
