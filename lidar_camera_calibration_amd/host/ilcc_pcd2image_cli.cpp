// ilcc_pcd2image -- ROS-free counterpart of the reference's pcd2image node (/root/reference/ilcc2/test/pcd2image.cpp):
// the first sensor_msgs/Image and the first PointCloud2 of a bag (or of two bags), the image undistorted in colour with
// the yaml's K and d, every LiDAR point that the extrinsic projects into it drawn as a dot coloured by intensity, and the
// picture written as a binary PPM in place of cv::imshow.
//   ilcc_pcd2image --bag B [--lidar-bag L] --image-topic T --lidar-topic T --yaml Y --extrinsic pose.bin --out out.ppm
//                  [--distance-valid 5] [--jpg-out out.jpg] [--quality 95]
// --jpg-out writes the same picture as a JPEG file too (include/ilcc_jpeg_write.h: what cv::imwrite would write for it,
// 4:2:0); both files show one picture.
// The file shows what the reference's window showed, red and blue swapped included (include/ilcc_overlay.h).
//   ilcc_pcd2image --all-pairs --jpg-out-all PREFIX [--ppm-out-all PREFIX] [--max-dt-ms 50] [--first N] [--stride N] [--max-scans N]
//                  [--huffman gpu|host] + the bag, topic, yaml and extrinsic arguments above (no --out)
// is the node over the whole recording (include/ilcc_overlay_sequence.h): every cloud message drawn on the image whose header stamp
// is nearest to its own, written as PREFIX<cloud message, 6 digits>.jpg (and .ppm), one line per scan.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ilcc_calib.h"
#include "ilcc_hip.h"
#include "ilcc_jpeg_write.h"
#include "ilcc_overlay.h"
#include "ilcc_overlay_sequence.h"

namespace {

constexpr const char* kUsage =
    "usage: ilcc_pcd2image --bag file.bag [--lidar-bag lidar.bag] --image-topic /camera/image_raw "
    "--lidar-topic /velodyne_points --yaml camera.yaml --extrinsic pose.bin --out out.ppm "
    "[--distance-valid 5] [--jpg-out out.jpg] [--quality 95]\n"
    "       ilcc_pcd2image --all-pairs --jpg-out-all PREFIX [--ppm-out-all PREFIX] [--max-dt-ms 50] [--first N] [--stride N] "
    "[--max-scans N] [--huffman gpu|host] --bag ... --image-topic ... --lidar-topic ... --yaml ... --extrinsic ... "
    "[--lidar-bag ...] [--distance-valid 5] [--quality 95]\n";

struct AllPairs {
  std::string jpg_prefix, ppm_prefix;
  int32_t width = 0, height = 0;
  bool failed = false;
};

std::string numbered(const std::string& prefix, uint32_t message, const char* ext) {
  char number[16];
  std::snprintf(number, sizeof(number), "%06u", (unsigned)message);
  return prefix + number + ext;
}

// one line per scan; the files of a paired one
int32_t on_scan(void* user, const ilcc_overlay_record* r, const uint8_t* jpeg, uint64_t jpeg_bytes, const uint8_t* bgr) {
  AllPairs* A = static_cast<AllPairs*>(user);
  if (r->image_message < 0) {
    std::printf("cloud %u: no image within the limit (nearest dt %.3f ms)\n", r->message, (double)r->dt_ns / 1e6);
    return 0;
  }
  const std::string jpg = numbered(A->jpg_prefix, r->message, ".jpg");
  FILE* f = std::fopen(jpg.c_str(), "wb");
  bool ok = f != nullptr;
  if (f) {
    ok = std::fwrite(jpeg, 1, jpeg_bytes, f) == jpeg_bytes;
    ok = (std::fclose(f) == 0) && ok;
  }
  if (ok && bgr && !A->ppm_prefix.empty()) ok = ilcc_save_ppm_bgr(numbered(A->ppm_prefix, r->message, ".ppm").c_str(), bgr, A->width, A->height) == ILCC_OK;
  if (!ok) {
    std::fprintf(stderr, "can not write the files of cloud %u\n", r->message);
    A->failed = true;
    return 1;
  }
  std::printf("cloud %u: image %d, dt %.3f ms, %llu points, %u drawn -> %s (%llu bytes, %s)\n", r->message, r->image_message, (double)r->dt_ns / 1e6,
              (unsigned long long)r->n_points, r->n_drawn, jpg.c_str(), (unsigned long long)r->file_bytes, r->route ? "host" : "gpu");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  std::string bag_path, lidar_bag_path, image_topic, lidar_topic, yaml_path, extrinsic_path, out_path, jpg_out_path, huffman = "gpu";
  bool all_pairs = false;
  AllPairs all;
  ilcc_overlay_sequence_params sp;
  ilcc_default_overlay_sequence_params(&sp);
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
    else if (a == "--all-pairs") all_pairs = true;
    else if (a == "--jpg-out-all" && i + 1 < argc) all.jpg_prefix = argv[++i];
    else if (a == "--ppm-out-all" && i + 1 < argc) all.ppm_prefix = argv[++i];
    else if (a == "--max-dt-ms" && i + 1 < argc) sp.max_dt_ns = (uint64_t)(std::atof(argv[++i]) * 1e6);
    else if (a == "--first" && i + 1 < argc) sp.first = (uint32_t)std::strtoul(argv[++i], nullptr, 10);
    else if (a == "--stride" && i + 1 < argc) sp.stride = (uint32_t)std::strtoul(argv[++i], nullptr, 10);
    else if (a == "--max-scans" && i + 1 < argc) sp.max_scans = (uint32_t)std::strtoul(argv[++i], nullptr, 10);
    else if (a == "--huffman" && i + 1 < argc) huffman = argv[++i];
    else {
      std::fprintf(stderr, "unknown or incomplete argument: %s\n", a.c_str());
      return 2;
    }
  }
  const bool common = !bag_path.empty() && !image_topic.empty() && !lidar_topic.empty() && !yaml_path.empty() && !extrinsic_path.empty();
  const bool sequence_ok = all_pairs && !all.jpg_prefix.empty() && out_path.empty() && jpg_out_path.empty() && (huffman == "gpu" || huffman == "host");
  const bool sequence_only = !all.jpg_prefix.empty() || !all.ppm_prefix.empty();   // the prefixes mean nothing without --all-pairs
  if (!common || (all_pairs ? !sequence_ok : (out_path.empty() || sequence_only))) {
    std::fprintf(stderr, "%s", kUsage);
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
  if (all_pairs) {
    sp.route = huffman == "host" ? 1u : 0u;
    sp.keep_pixels = all.ppm_prefix.empty() ? 0u : 1u;
    all.width = cam.width;
    all.height = cam.height;
    uint32_t n_scans = 0, n_paired = 0;
    const int32_t st = ilcc_bag_pcd2image_all_pairs(0, bag_path.c_str(), image_topic.c_str(), lidar_bag_path.c_str(), lidar_topic.c_str(), &cam, T,
                                                    distance_valid, quality, &sp, on_scan, &all, &n_scans, &n_paired);
    if (st != ILCC_OK) {
      std::fprintf(stderr, "%s: %s\n", all.failed ? "can not write" : "can't read lidar or image topic", ilcc_last_error(nullptr));
      return 1;
    }
    std::printf("%u scans, %u paired -> %s*.jpg\n", n_scans, n_paired, all.jpg_prefix.c_str());
    return 0;
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
