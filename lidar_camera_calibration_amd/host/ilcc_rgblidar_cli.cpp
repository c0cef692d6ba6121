// ilcc_rgblidar -- ROS-free counterpart of the reference's rgblidar node (ilcc2/test/rgblidar.cpp) over a WHOLE recording: every
// PointCloud2 of the LiDAR topic is coloured from the sensor_msgs/Image whose header stamp is nearest to its own (within --max-dt-ms)
// and written as out-dir/rgb_lidar_<k>.pcd, k counting the paired scans; --merged writes all of them as one cloud, which for a static
// rig is the most telling picture of the extrinsic (include/ilcc_paired.h).
//   ilcc_rgblidar --image-bag B --image-topic T --lidar-bag L --lidar-topic T --yaml Y --extrinsic pose.bin --out-dir D
//                 [--merged file.pcd] [--max-dt-ms 50] [--distance-valid 5] [--raw-image] [--first 0] [--stride 1] [--max-scans 0]
// The image is undistorted with the yaml's K and d before it is sampled; --raw-image samples it as the bag carries it, which is
// what the reference does.  One line per scan: message, image message, dt, points, coloured.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ilcc_calib.h"
#include "ilcc_hip.h"
#include "ilcc_paired.h"

namespace {

struct Writer {
  std::string out_dir;
  bool merge = false;
  uint32_t written = 0;
  std::vector<uint8_t> merged;
};

int32_t on_scan(void* user, const ilcc_pair_record* r, const void* xyzrgb) {
  Writer* w = static_cast<Writer*>(user);
  if (r->image_message < 0) {
    std::printf("cloud %u: no image within the limit (nearest dt %.3f ms), %" PRIu64 " points\n", r->message, r->dt_ns * 1e-6, r->n_points);
    return 0;
  }
  const std::string path = w->out_dir + "/rgb_lidar_" + std::to_string(w->written) + ".pcd";
  if (ilcc_save_pcd_xyzrgb(path.c_str(), xyzrgb, r->n_coloured) != ILCC_OK) {
    std::fprintf(stderr, "can not write %s\n", path.c_str());
    return 1;
  }
  ++w->written;
  if (w->merge) {
    const uint8_t* p = static_cast<const uint8_t*>(xyzrgb);
    w->merged.insert(w->merged.end(), p, p + 16 * r->n_coloured);
  }
  std::printf("cloud %u: image %d, dt %.3f ms, %" PRIu64 " points, %" PRIu64 " coloured -> %s\n", r->message, r->image_message, r->dt_ns * 1e-6,
              r->n_points, r->n_coloured, path.c_str());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  std::string image_bag, lidar_bag, image_topic, lidar_topic, yaml_path, extrinsic_path, out_dir, merged_path;
  double distance_valid = 5, max_dt_ms = 50;   // rgblidar.cpp:112
  ilcc_paired_params pp;
  ilcc_default_paired_params(&pp);
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--image-bag" && i + 1 < argc) image_bag = argv[++i];
    else if (a == "--lidar-bag" && i + 1 < argc) lidar_bag = argv[++i];
    else if (a == "--image-topic" && i + 1 < argc) image_topic = argv[++i];
    else if (a == "--lidar-topic" && i + 1 < argc) lidar_topic = argv[++i];
    else if (a == "--yaml" && i + 1 < argc) yaml_path = argv[++i];
    else if (a == "--extrinsic" && i + 1 < argc) extrinsic_path = argv[++i];
    else if (a == "--out-dir" && i + 1 < argc) out_dir = argv[++i];
    else if (a == "--merged" && i + 1 < argc) merged_path = argv[++i];
    else if (a == "--max-dt-ms" && i + 1 < argc) max_dt_ms = std::atof(argv[++i]);
    else if (a == "--distance-valid" && i + 1 < argc) distance_valid = std::atof(argv[++i]);
    else if (a == "--raw-image") pp.sample_raw = 1;
    else if (a == "--first" && i + 1 < argc) pp.first = (uint32_t)std::strtoul(argv[++i], nullptr, 10);
    else if (a == "--stride" && i + 1 < argc) pp.stride = (uint32_t)std::strtoul(argv[++i], nullptr, 10);
    else if (a == "--max-scans" && i + 1 < argc) pp.max_scans = (uint32_t)std::strtoul(argv[++i], nullptr, 10);
    else {
      std::fprintf(stderr, "unknown or incomplete argument: %s\n", a.c_str());
      return 2;
    }
  }
  if (image_bag.empty() || lidar_bag.empty() || image_topic.empty() || lidar_topic.empty() || yaml_path.empty() || extrinsic_path.empty() ||
      out_dir.empty() || !(max_dt_ms >= 0)) {
    std::fprintf(stderr, "usage: ilcc_rgblidar --image-bag file.bag --image-topic /camera/image_raw --lidar-bag file.bag --lidar-topic /velodyne_points "
                         "--yaml camera.yaml --extrinsic pose.bin --out-dir dir [--merged file.pcd] [--max-dt-ms 50] [--distance-valid 5] "
                         "[--raw-image] [--first 0] [--stride 1] [--max-scans 0]\n");
    return 2;
  }
  pp.max_dt_ns = (uint64_t)(max_dt_ms * 1e6 + 0.5);
  ilcc_camera_model cam;
  if (ilcc_read_camera_yaml(yaml_path.c_str(), &cam) != ILCC_OK) {
    std::fprintf(stderr, "%s\n", ilcc_last_error(nullptr));
    return 1;
  }
  double T[16];
  if (ilcc_extrinsic_read(extrinsic_path.c_str(), T) != 0) {
    std::fprintf(stderr, "can not open %s\n", extrinsic_path.c_str());
    return 1;
  }
  Writer w;
  w.out_dir = out_dir;
  w.merge = !merged_path.empty();
  uint32_t n_scans = 0, n_paired = 0;
  const int32_t st = ilcc_bag_rgblidar_all_scans(0, image_bag.c_str(), image_topic.c_str(), lidar_bag.c_str(), lidar_topic.c_str(), &cam, T, distance_valid,
                                                 &pp, on_scan, &w, &n_scans, &n_paired);
  if (st != ILCC_OK) {
    std::fprintf(stderr, "can't read lidar or image topic: %s\n", ilcc_last_error(nullptr));
    return 1;
  }
  if (w.merge) {
    if (ilcc_save_pcd_xyzrgb(merged_path.c_str(), w.merged.data(), w.merged.size() / 16) != ILCC_OK) {
      std::fprintf(stderr, "can not write %s\n", merged_path.c_str());
      return 1;
    }
    std::printf("merged %zu points -> %s\n", w.merged.size() / 16, merged_path.c_str());
  }
  std::printf("%u scans, %u paired\n", n_scans, n_paired);
  return 0;
}
