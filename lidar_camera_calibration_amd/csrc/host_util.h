// What the host chains (bag -> parser -> one hipMalloc -> kernels -> result) share: the last-error text behind a status,
// the 256-byte alignment of the parts of a device buffer, a device buffer freed on scope exit, the device check, the first
// message of a bag topic in a vector, and the std_msgs/Header every ROS message starts with; and what the chains over every
// message of a topic share: the scope guards, the md5 sums of the two image types, message i in a vector, the first / stride / max
// selection and the image-topic open with its CompressedImage refusal.  Internal, not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "ilcc_hip.h"
#include "ilcc_ingest.h"
#include "ilcc_sequence.h"   // the topic iterator

namespace ilcc {

void set_global_error(const std::string& s);   // ilcc_api.cpp: the text behind ilcc_last_error(NULL)

inline int32_t fail(int32_t code, const std::string& what) {
  set_global_error(what);
  return code;
}

inline int32_t hip_fail(hipError_t e) { return fail(ILCC_HIP_ERROR, std::string("hip: ") + hipGetErrorString(e)); }

inline uint64_t align256(uint64_t bytes) { return (bytes + 255u) & ~(uint64_t)255u; }   // every part of a device buffer starts on a 256-byte boundary

struct DeviceBuffer {
  void* p = nullptr;
  ~DeviceBuffer() {
    if (p) (void)hipFree(p);
  }
};

inline int32_t no_device() { return fail(ILCC_HIP_ERROR, "no HIP device: libilcc_hip has no CPU fallback"); }

// makes `device` the current one; a chain calls it after its host-side refusals and before its first allocation
inline int32_t select_device(int32_t device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return no_device();
  const hipError_t e = hipSetDevice(device);
  return e == hipSuccess ? ILCC_OK : hip_fail(e);
}

// the first message on `topic` whose connection carries md5 (nullptr: PointCloud2's)
inline int32_t read_first_message(const char* bag_path, const char* topic, const char* md5, std::vector<uint8_t>* msg) {
  uint64_t bytes = 0;
  const int32_t st = ilcc_bag_first_message(bag_path, topic, md5, nullptr, 0, &bytes);
  if (st != ILCC_CAPACITY && st != ILCC_OK) return st;
  try {
    msg->resize(bytes);
  } catch (...) {   // no exception crosses the C-ABI
    return fail(ILCC_IO_ERROR, "out of memory for the bag's message");
  }
  return ilcc_bag_first_message(bag_path, topic, md5, msg->data(), bytes, &bytes);
}

// ---- what the chains over every message of a topic share (the six *_api.cpp chain files)

constexpr const char* kImageMd5 = "060021388200f6f0f447d0fcd9c64743";             // sensor_msgs/Image
constexpr const char* kCompressedImageMd5 = "8f7a12909da2c9d3332d540a0977563f";   // sensor_msgs/CompressedImage

inline uint64_t align16(uint64_t v) { return (v + 15u) & ~(uint64_t)15u; }
inline uint64_t stamp_ns(uint32_t sec, uint32_t nsec) { return (uint64_t)sec * 1000000000ull + nsec; }

struct Iterator {
  ilcc_bag_topic* it = nullptr;
  ~Iterator() { ilcc_bag_topic_close(it); }
};
struct Stream {
  hipStream_t s = nullptr;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
};
struct Pinned {
  uint8_t* p = nullptr;
  ~Pinned() {
    if (p) (void)hipHostFree(p);
  }
};
// whatever made the call end, the stream's work must have finished before the buffers it uses go away: declared behind them
struct InFlight {
  hipStream_t s = nullptr;
  ~InFlight() {
    if (s) (void)hipStreamSynchronize(s);
  }
};

// the message `i` of the topic in `msg` (never empty, so that data() is an address), its length in *bytes
inline int32_t read_message(ilcc_bag_topic* it, uint64_t i, std::vector<uint8_t>* msg, uint64_t* bytes) {
  const int32_t st = ilcc_bag_topic_read(it, i, nullptr, 0, bytes);
  if (st != ILCC_OK && st != ILCC_CAPACITY) return st;
  msg->resize(*bytes ? *bytes : 1);
  return ilcc_bag_topic_read(it, i, msg->data(), *bytes, bytes);
}

// the message indices first, first + stride, ... of the topic, at most max of them (0: all); max_word names max in the refusal
inline int32_t select_messages(ilcc_bag_topic* it, uint64_t first, uint64_t stride, uint64_t max, const char* max_word, std::vector<uint64_t>* selected) {
  const uint64_t count = ilcc_bag_topic_count(it);
  for (uint64_t i = first; i < count && (max == 0 || selected->size() < max); i += stride ? stride : 1) selected->push_back(i);
  if (selected->empty()) return fail(ILCC_BAD_ARGUMENT, std::string("first / stride / ") + max_word + " select no message of the topic");
  return ILCC_OK;
}

// opens the topic's sensor_msgs/Image messages; a topic that carries only the compressed type is refused in `entry`'s name, with
// `hint` (a sentence that starts with ", ", or "") behind it
inline int32_t open_image_topic(const char* bag_path, const char* topic, const char* entry, const char* hint, ilcc_bag_topic** it) {
  const int32_t st = ilcc_bag_topic_open(bag_path, topic, kImageMd5, it);
  if (st != ILCC_BAD_ARGUMENT) return st;
  Iterator compressed;   // no sensor_msgs/Image there: say so when the topic carries the compressed type instead
  if (ilcc_bag_topic_open(bag_path, topic, kCompressedImageMd5, &compressed.it) == ILCC_OK)
    return fail(ILCC_BAD_ARGUMENT, std::string("topic ") + topic + " carries only sensor_msgs/CompressedImage: " + entry + " takes sensor_msgs/Image" + hint);
  return ilcc_bag_topic_open(bag_path, topic, kImageMd5, &compressed.it);   // the first refusal, with its text
}

inline bool read_u32(const uint8_t* m, uint64_t n, uint64_t* at, uint32_t* v) {
  if (*at > n || n - *at < 4) return false;
  std::memcpy(v, m + *at, 4);
  *at += 4;
  return true;
}

// std_msgs/Header at m[*at]: seq, stamp, frame_id (cut to 63 bytes; the caller has zeroed it).  false: the message ends inside it
inline bool read_header(const uint8_t* m, uint64_t n, uint64_t* at, uint32_t* seq, uint32_t* sec, uint32_t* nsec, char (&frame_id)[64]) {
  uint32_t len = 0;
  if (!read_u32(m, n, at, seq) || !read_u32(m, n, at, sec) || !read_u32(m, n, at, nsec) || !read_u32(m, n, at, &len) || len > n - *at)
    return false;
  std::memcpy(frame_id, m + *at, len < sizeof(frame_id) - 1 ? len : sizeof(frame_id) - 1);
  *at += len;
  return true;
}

}  // namespace ilcc
