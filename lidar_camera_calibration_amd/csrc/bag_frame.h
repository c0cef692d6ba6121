// The first frame of a camera topic, as its publisher encoded it: the first sensor_msgs/Image, or, when the topic carries
// none, the first sensor_msgs/CompressedImage, which K13 decodes.  ONE helper for ilcc_bag_first_image,
// ilcc_bag_find_chessboard and ilcc_bag_pcd2image (csrc/jpeg_host.cpp), in two steps so that a caller can check its own
// capacity and make its one hipMalloc between them; bag_image_to_device is those steps with K11 behind them, for
// ilcc_bag_first_image, ilcc_bag_find_chessboard and ilcc_bag_save_jpeg.
#ifndef ILCC_BAG_FRAME_H_
#define ILCC_BAG_FRAME_H_

#include <cstdint>
#include <vector>

#include "host_util.h"
#include "ilcc_jpeg.h"

namespace ilcc {

// where the coefficients and the kernel's scratch (`scratch`: the bytes K13 or K14 asks for) lie behind `pixel_bytes` of pixels
struct JpegLayout {
  uint64_t coef_at, scratch_at, scratch_bytes, total;
  JpegLayout(const ilcc_jpeg_info& I, uint64_t pixel_bytes, uint64_t scratch) {
    coef_at = align256(pixel_bytes);
    scratch_at = coef_at + align256(I.coef_count * sizeof(int16_t));
    scratch_bytes = scratch;
    total = scratch_at + align256(scratch_bytes);
  }
};

struct BagFrame {
  std::vector<uint8_t> msg;     // the serialized message
  bool compressed = false;
  ilcc_image_layout L{};        // of the pixels on the device: width, height, step, encoding (data_offset / data_bytes: in msg)
  ilcc_jpeg_info jpeg{};        // compressed only
  uint64_t device_bytes = 0;    // what bag_frame_to_device needs at d_mem
};

// host only: reads and parses the message (for a CompressedImage the JPEG headers too)
int32_t bag_frame_read(const char* bag_path, const char* topic, BagFrame* out);

// d_mem: frame.device_bytes of device memory on a 256-byte boundary.  Leaves the pixels at d_mem, rows L.step apart, in
// L.encoding, queued on the default stream of the current device (an Image: one H2D copy of data[]; a CompressedImage:
// entropy decode here, H2D of the coefficients, K13; coefficients and scratch lie behind the pixels).
int32_t bag_frame_to_device(const BagFrame& frame, void* d_mem);

// the first frame of the bag's topic on the device, converted: ONE device buffer holds the frame as the bag carries it
// (data[] of an Image, or what K13 makes of a CompressedImage), behind it the mono8 image, and behind that `extra`
struct DeviceImage {
  DeviceBuffer buffer;
  uint8_t* mono8 = nullptr;     // width x height, packed
  uint8_t* extra = nullptr;     // what extra_for asked for, on a 256-byte boundary; null when it asked for none
  ilcc_image_layout L{};
};

// bag_frame_read -> one hipMalloc -> bag_frame_to_device -> K11 (mono8; undistorted when a camera is given), all queued on
// the default stream of `device` (csrc/camera_image_host.cpp).  cap_pixels: refuse with ILCC_CAPACITY (*width, *height
// reported) before the GPU is touched when the image is larger.  extra_for, when given, says how many bytes of its own the
// caller wants in the same allocation for an image of that size (0: none).
int32_t bag_image_to_device(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera,
                            uint64_t cap_pixels, uint64_t (*extra_for)(int32_t width, int32_t height), int32_t* width, int32_t* height,
                            DeviceImage* out);

}  // namespace ilcc

#endif
