// What the host chains (bag -> parser -> one hipMalloc -> kernels -> result) share: the last-error text behind a status,
// the 256-byte alignment of the parts of a device buffer, a device buffer freed on scope exit, the device check, the first
// message of a bag topic in a vector, and the std_msgs/Header every ROS message starts with.  Internal, not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "ilcc_hip.h"
#include "ilcc_ingest.h"

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
