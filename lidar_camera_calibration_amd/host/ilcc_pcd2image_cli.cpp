// ilcc_pcd2image -- ROS-free counterpart of the reference's pcd2image node (/root/reference/ilcc2/test/pcd2image.cpp):
// the first sensor_msgs/Image and the first PointCloud2 of a bag (or of two bags), the image undistorted in colour with
// the yaml's K and d, every LiDAR point that the extrinsic projects into it drawn as a dot coloured by intensity, and the
// picture written as a binary PPM in place of cv::imshow.
//   ilcc_pcd2image --bag B [--lidar-bag L] --image-topic T --lidar-topic T --yaml Y --extrinsic pose.bin --out out.ppm
//                  [--distance-valid 5] [--jpg-out out.jpg] [--quality 95]
// --jpg-out writes the same picture as a JPEG file too (include/ilcc_jpeg_write.h: what cv::imwrite would write for it,
// 4:2:0); both files show one picture.
// The file shows what the reference's window showed, red and blue swapped included (include/ilcc_overlay.h).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ilcc_calib.h"
#include "ilcc_hip.h"
#include "ilcc_jpeg_write.h"
#include "ilcc_overlay.h"

int main(int argc, char** argv) {
  std::string bag_path, lidar_bag_path, image_topic, lidar_topic, yaml_path, extrinsic_path, out_path, jpg_out_path;
  int quality = 95;
  double distance_valid = 5;   // pcd2image.cpp:122
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--bag" && i + 1 < argc) bag_path = argv[++i];
    else if (a == "--lidar-bag" && i + 1 < argc) lidar_bag_path = argv[++i];
    else if (a == "--image-topic" && i + 1 < argc) image_topic = argv[++i];
    else if (a == "--lidar-topic" && i + 1 < argc) lidar_topic = argv[++i];
    else if (a == "--yaml" && i + 1 < argc) yaml_path = argv[++i];
    else if (a == "--extrinsic" && i + 1 < argc) extrinsic_path = argv[++i];
    else if (a == "--out" && i + 1 < argc) out_path = argv[++i];
    else if (a == "--distance-valid" && i + 1 < argc) distance_valid = std::atof(argv[++i]);
    else if (a == "--jpg-out" && i + 1 < argc) jpg_out_path = argv[++i];
    else if (a == "--quality" && i + 1 < argc) quality = std::atoi(argv[++i]);
    else {
      std::fprintf(stderr, "unknown or incomplete argument: %s\n", a.c_str());
      return 2;
    }
  }
  if (bag_path.empty() || image_topic.empty() || lidar_topic.empty() || yaml_path.empty() || extrinsic_path.empty() || out_path.empty()) {
    std::fprintf(stderr, "usage: ilcc_pcd2image --bag file.bag [--lidar-bag lidar.bag] --image-topic /camera/image_raw "
                         "--lidar-topic /velodyne_points --yaml camera.yaml --extrinsic pose.bin --out out.ppm "
                         "[--distance-valid 5] [--jpg-out out.jpg] [--quality 95]\n");
    return 2;
  }
  if (lidar_bag_path.empty()) lidar_bag_path = bag_path;
  ilcc_camera_model cam;
  if (ilcc_read_camera_yaml(yaml_path.c_str(), &cam) != ILCC_OK) {
    std::fprintf(stderr, "%s\n", ilcc_last_error(nullptr));   // "can not open ..." as ImageCornersEst.cpp:20-24
    return 1;
  }
  double T[16];
  if (ilcc_extrinsic_read(extrinsic_path.c_str(), T) != 0) {
    std::fprintf(stderr, "can not open %s\n", extrinsic_path.c_str());
    return 1;
  }
  int32_t w = 0, h = 0;
  uint32_t drawn = 0;
  std::vector<uint8_t> pixels((size_t)cam.width * (size_t)cam.height * 3);
  const int32_t st = ilcc_bag_pcd2image(0, bag_path.c_str(), image_topic.c_str(), lidar_bag_path.c_str(), lidar_topic.c_str(), &cam,
                                        T, distance_valid, pixels.data(), pixels.size(), &w, &h, &drawn);
  if (st != ILCC_OK) {
    std::fprintf(stderr, "can't read lidar or image topic: %s\n", ilcc_last_error(nullptr));
    return 1;
  }
  if (ilcc_save_ppm_bgr(out_path.c_str(), pixels.data(), w, h) != ILCC_OK) {
    std::fprintf(stderr, "can not write %s\n", out_path.c_str());
    return 1;
  }
  std::printf("image %d x %d, %u points drawn -> %s\n", w, h, drawn, out_path.c_str());
  if (!jpg_out_path.empty()) {
    if (ilcc_jpeg_write_file(0, jpg_out_path.c_str(), pixels.data(), 3 * w, w, h, ILCC_ENCODING_BGR8, quality) != ILCC_OK) {
      std::fprintf(stderr, "can not write %s: %s\n", jpg_out_path.c_str(), ilcc_last_error(nullptr));
      return 1;
    }
    std::printf("quality %d -> %s\n", quality, jpg_out_path.c_str());
  }
  return 0;
}
