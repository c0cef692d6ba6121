// Host side of include/ilcc_overlay.h: pcd2image (/root/reference/ilcc2/test/pcd2image.cpp:33-104) from bags -- the first
// frame of the camera topic (csrc/bag_frame.h) and the first PointCloud2, H2D, K11c -> K0 -> K8 -> K12 on the default stream, D2H -- and the PPM writer that
// stands in for cv::imshow.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bag_frame.h"
#include "host_util.h"
#include "ilcc_hip.h"
#include "ilcc_ingest.h"
#include "ilcc_overlay.h"
#include "ilcc_project.h"

using namespace ilcc;

extern "C" {

int32_t ilcc_bag_pcd2image(int32_t device, const char* image_bag, const char* image_topic, const char* lidar_bag,
                           const char* lidar_topic, const ilcc_camera_model* camera, const double T[16], double distance_valid,
                           uint8_t* bgr_out, uint64_t cap_bytes, int32_t* width, int32_t* height, uint32_t* n_drawn) {
  if (!width || !height || !n_drawn || !camera || !T || (!bgr_out && cap_bytes))
    return fail(ILCC_BAD_ARGUMENT, "ilcc_bag_pcd2image: null argument");
  *width = *height = 0;
  *n_drawn = 0;
  std::vector<uint8_t> cloud_msg;
  BagFrame frame;
  int32_t st = bag_frame_read(image_bag, image_topic, &frame);
  if (st != ILCC_OK) return st;
  const ilcc_image_layout& I = frame.L;
  if (I.width > 65536u || I.height > 65536u) return fail(ILCC_BAD_ARGUMENT, "image larger than 65536 pixels a side");
  if (I.step > (uint32_t)INT32_MAX) return fail(ILCC_BAD_ARGUMENT, "image step too large");
  const int32_t w = (int32_t)I.width, h = (int32_t)I.height;
  *width = w;
  *height = h;
  const uint64_t bgr_bytes = 3ull * I.width * I.height;
  if (bgr_bytes > cap_bytes) return fail(ILCC_CAPACITY, "image larger than the buffer");
  if (camera->width != w || camera->height != h) return fail(ILCC_BAD_ARGUMENT, "the camera's width / height differ from the image's");
  st = read_first_message(lidar_bag, lidar_topic, nullptr, &cloud_msg);
  if (st != ILCC_OK) return st;
  ilcc_pointcloud2_layout P;
  st = ilcc_pointcloud2_parse(cloud_msg.data(), cloud_msg.size(), &P);
  if (st != ILCC_OK) return st;
  const uint64_t points = (uint64_t)P.height * P.width;
  if (points > 0xFFFFFFFEull) return fail(ILCC_BAD_ARGUMENT, "cloud of more than 2^32 - 2 points");
  st = select_device(device);
  if (st != ILCC_OK) return st;

  // ONE device buffer: [ the frame as the bag carries it | B,G,R image | cloud data[] | XYZI | hits | K12's owner words ]
  const uint64_t bgr_at = align256(frame.device_bytes);
  const uint64_t cloud_at = bgr_at + align256(bgr_bytes);
  const uint64_t xyzi_at = cloud_at + align256(P.data_bytes);
  const uint64_t hits_at = xyzi_at + align256(16 * points);
  const uint64_t owner_at = hits_at + align256(16 * points);
  const uint64_t total = owner_at + ilcc_draw_hits_scratch_bytes(w, h);
  DeviceBuffer buf;
  hipError_t e = hipMalloc(&buf.p, total);
  if (e != hipSuccess) return hip_fail(e);
  uint8_t* base = (uint8_t*)buf.p;
  st = bag_frame_to_device(frame, base);
  if (st != ILCC_OK) return st;
  st = ilcc_image_to_bgr8_device(base, w, h, (int32_t)I.step, (int32_t)I.encoding, camera, base + bgr_at, 3 * w, nullptr);
  if (st != ILCC_OK) return st;
  if (points) {
    e = hipMemcpy(base + cloud_at, cloud_msg.data() + P.data_offset, P.data_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e);
    st = ilcc_pointcloud2_unpack_device(base + cloud_at, &P, base + xyzi_at, nullptr);
    if (st != ILCC_OK) return st;
    const ilcc_projection proj = {{T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, {T[3], T[7], T[11]},
                                  camera->fx, camera->cx, camera->fy, camera->cy, w, h};
    uint32_t hits = 0;
    st = ilcc_project_intensity_device(base + xyzi_at, (uint32_t)points, &proj, distance_valid, 0.0, 60.0, base + hits_at, &hits,
                                       nullptr);   // pcd2image.cpp:53-54
    if (st != ILCC_OK) return st;
    st = ilcc_draw_hits_device(base + bgr_at, w, h, 3 * w, base + hits_at, hits, nullptr, 0, base + owner_at, nullptr);
    if (st != ILCC_OK) return st;
    *n_drawn = hits;
  }
  e = hipMemcpy(bgr_out, base + bgr_at, bgr_bytes, hipMemcpyDeviceToHost);   // waits for the kernels
  if (e != hipSuccess) return hip_fail(e);
  return ILCC_OK;
}

int32_t ilcc_save_ppm_bgr(const char* filename, const uint8_t* bgr, int32_t width, int32_t height) {
  if (!filename || !bgr || width < 1 || height < 1) return fail(ILCC_BAD_ARGUMENT, "ilcc_save_ppm_bgr: bad argument");
  FILE* f = std::fopen(filename, "wb");
  if (!f) return fail(ILCC_IO_ERROR, std::string("can not write ") + filename);
  bool ok = std::fprintf(f, "P6\n%d %d\n255\n", width, height) > 0;
  try {
    std::vector<uint8_t> row((size_t)width * 3);
    for (int32_t i = 0; i < height && ok; ++i) {
      const uint8_t* p = bgr + (size_t)i * row.size();
      for (int32_t j = 0; j < width; ++j) {
        row[3 * j] = p[3 * j + 2];
        row[3 * j + 1] = p[3 * j + 1];
        row[3 * j + 2] = p[3 * j];
      }
      ok = std::fwrite(row.data(), 1, row.size(), f) == row.size();
    }
  } catch (...) {   // no exception crosses the C-ABI
    ok = false;
  }
  ok = (std::fclose(f) == 0) && ok;
  return ok ? ILCC_OK : fail(ILCC_IO_ERROR, std::string("can not write ") + filename);
}

}  // extern "C"
