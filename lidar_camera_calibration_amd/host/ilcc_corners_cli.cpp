// ilcc_corners -- ROS-free driver of the get_lidar_corners path for machines without ROS (the GPU
// box): one frame (raw float32 x,y,z,intensity records) + one click -> process_data-format file.
//   ilcc_corners --cloud frame.bin --click x y z --yaml pointgrey.yaml --out pointgrey_lidar_1.txt
//                [--solver grid|reference] [--device N] [--accept-ambiguous] [--accept-low-coverage]
//   ilcc_corners --bag 20181101_1.bag [--topic /velodyne_points] --click x y z ... (first PointCloud2
//                of the bag, read without ROS: include/ilcc_ingest.h)
//   --auto in place of --click x y z: the seed is proposed from the cloud itself (include/ilcc_seed.h) and printed
//   --auto-planar likewise, from planar seeds: for a board that stands on the floor, on a stand or in a hand
//   --bag ... --all-scans [--first i] [--stride k] [--max-scans n] [--gate metres] [--report file]: every PointCloud2 of the topic
//                (include/ilcc_sequence.h), the accepted scans' corners fused into ONE set, written in the same format
// Mirrors the per-bag body of /root/reference/ilcc2/test/get_lidar_corners.cpp:133-204.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "LidarCornersEst.h"
#include "ilcc_ingest.h"
#include "ilcc_sequence.h"

using namespace ilcc_host;

namespace {

struct AllScans {
  bool on = false;
  ilcc_sequence_params sp;
  std::string report;
};

// --all-scans: the whole topic through one handle sized from the bag's first cloud
int run_all_scans(const AllScans& a, const std::string& bag_path, const std::string& topic, const std::string& yaml_path, const std::string& out_path,
                  const std::string& solver, int device, const float* click, int seed_mode) {
  ilcc_params p;
  ilcc_default_params(&p);
  p.solver = (solver == "reference") ? ILCC_SOLVER_REFERENCE_LOCAL : ILCC_SOLVER_GRID;
  if (!yaml_path.empty() && ilcc_set_chessboard_param(&p, yaml_path.c_str()) != ILCC_OK) {
    std::fprintf(stderr, "can not open %s\n", yaml_path.c_str());
    return 1;
  }
  ilcc_bag_topic* it = nullptr;
  if (ilcc_bag_topic_open(bag_path.c_str(), topic.c_str(), nullptr, &it) != ILCC_OK) {
    std::fprintf(stderr, "can't read lidar topic: %s\n", ilcc_last_error(nullptr));
    return 1;
  }
  const uint64_t count = ilcc_bag_topic_count(it);
  uint64_t largest = 0;
  for (uint64_t i = 0; i < count; ++i) {
    uint64_t bytes = 0;
    (void)ilcc_bag_topic_read(it, i, nullptr, 0, &bytes);
    if (bytes > largest) largest = bytes;
  }
  ilcc_bag_topic_close(it);
  // the handle: up to 64 frames per batch (at least the 4 candidates of a seed search), each of up to 1/16 of the largest
  // message's bytes in points -- a velodyne point takes 32 bytes, a packed x y z intensity point 16; denser clouds are ILCC_CAPACITY
  const uint32_t frames = (uint32_t)(count < 64 ? (count < 4 ? 4 : count) : 64);
  const uint64_t points_per_frame = largest / 16 + 1024;
  ilcc_handle* h = ilcc_create(device, &p, frames, frames * points_per_frame);
  if (!h) {
    std::fprintf(stderr, "ilcc_create: %s\n", ilcc_last_error(nullptr));
    return 1;
  }
  std::vector<ilcc_scan_record> scans(count);
  ilcc_sequence_result r;
  const int32_t st = ilcc_bag_corners_all_scans(h, bag_path.c_str(), topic.c_str(), click, seed_mode, &a.sp, &r, scans.data(), (uint32_t)count);
  int rc = 0;
  if (st == ILCC_BOARD_NOT_FOUND && seed_mode != ILCC_SEED_CLICK && r.n_ok == 0 && r.n_batches == 0) {
    std::printf("no chessboard found\n");
    rc = 3;
  } else if (st != ILCC_OK && st != ILCC_AMBIGUOUS && st != ILCC_BOARD_NOT_FOUND) {
    std::fprintf(stderr, "all scans: %s: %s\n", ilcc_strerror(st), ilcc_last_error(nullptr));
    rc = 1;
  } else {
    if (seed_mode != ILCC_SEED_CLICK) std::printf("seed %.9g %.9g %.9g\n", r.click[0], r.click[1], r.click[2]);
    if (!a.report.empty()) {
      std::FILE* f = std::fopen(a.report.c_str(), "w");
      if (!f) {
        std::fprintf(stderr, "can not write %s\n", a.report.c_str());
        ilcc_destroy(h);
        return 1;
      }
      for (int32_t s = 0; s < r.n_scans; ++s)
        std::fprintf(f, "scan %d message %u stamp %u.%09u status %d flags %d used %d distance_mm %.3f\n", s, scans[s].message, scans[s].stamp_sec,
                     scans[s].stamp_nsec, scans[s].result.status, scans[s].result.flags, scans[s].used,
                     scans[s].distance < 0 ? -1.0 : scans[s].distance * 1e3);
      std::fclose(f);
    }
    if (st == ILCC_OK) {
      std::cout << "add_corner" << std::endl;
      if (ilcc_save_corners2txt(r.corners, (uint32_t)r.n_corners, out_path.c_str()) != ILCC_OK) {
        std::fprintf(stderr, "can not write %s\n", out_path.c_str());
        rc = 1;
      }
    } else {
      rc = 4;
    }
    std::printf("all scans: status %d scans %d accepted %d used %d batches %d spread_rms_mm %.3f spread_max_mm %.3f ref_scan %d corners %d -> %s\n", st,
                r.n_scans, r.n_ok, r.n_used, r.n_batches, r.spread_rms * 1e3, r.spread_max * 1e3, r.ref_scan, r.n_corners,
                st == ILCC_OK && rc == 0 ? out_path.c_str() : "-");
  }
  ilcc_destroy(h);
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  std::string cloud_path, bag_path, topic = "/velodyne_points", yaml_path, out_path, solver = "grid";
  PointXYZI click{0, 0, 0, 0};
  int device = -1;
  AllScans all;
  ilcc_default_sequence_params(&all.sp);
  bool have_click = false, auto_seed = false, auto_planar = false, accept_ambiguous = false, accept_low_coverage = false;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--cloud" && i + 1 < argc) cloud_path = argv[++i];
    else if (a == "--bag" && i + 1 < argc) bag_path = argv[++i];
    else if (a == "--topic" && i + 1 < argc) topic = argv[++i];
    else if (a == "--yaml" && i + 1 < argc) yaml_path = argv[++i];
    else if (a == "--out" && i + 1 < argc) out_path = argv[++i];
    else if (a == "--solver" && i + 1 < argc) solver = argv[++i];
    else if (a == "--device" && i + 1 < argc) device = std::atoi(argv[++i]);
    else if (a == "--accept-ambiguous") accept_ambiguous = true;
    else if (a == "--accept-low-coverage") accept_low_coverage = true;
    else if (a == "--all-scans") all.on = true;
    else if (a == "--first" && i + 1 < argc) all.sp.first = (uint32_t)std::strtoul(argv[++i], nullptr, 10);
    else if (a == "--stride" && i + 1 < argc) all.sp.stride = (uint32_t)std::strtoul(argv[++i], nullptr, 10);
    else if (a == "--max-scans" && i + 1 < argc) all.sp.max_scans = (uint32_t)std::strtoul(argv[++i], nullptr, 10);
    else if (a == "--gate" && i + 1 < argc) all.sp.gate = std::atof(argv[++i]);
    else if (a == "--report" && i + 1 < argc) all.report = argv[++i];
    else if (a == "--auto") auto_seed = true;
    else if (a == "--auto-planar") auto_planar = true;
    else if (a == "--click" && i + 3 < argc) {
      click.x = (float)std::atof(argv[++i]);
      click.y = (float)std::atof(argv[++i]);
      click.z = (float)std::atof(argv[++i]);
      have_click = true;
    } else {
      std::fprintf(stderr, "unknown or incomplete argument: %s\n", a.c_str());
      return 2;
    }
  }
  if ((cloud_path.empty() == bag_path.empty()) || out_path.empty() || (int)have_click + (int)auto_seed + (int)auto_planar != 1) {
    std::fprintf(stderr, "usage: ilcc_corners (--cloud frame.bin | --bag file.bag [--topic /velodyne_points]) (--click x y z | --auto | --auto-planar) "
                         "[--yaml board.yaml] --out file.txt [--solver grid|reference] [--device N] [--accept-ambiguous] [--accept-low-coverage] "
                         "[--all-scans [--first i] [--stride k] [--max-scans n] [--gate metres] [--report file]]\n");
    return 2;
  }
  if (all.on) {
    if (bag_path.empty()) {
      std::fprintf(stderr, "--all-scans needs --bag\n");
      return 2;
    }
    all.sp.accept_ambiguous = accept_ambiguous;
    all.sp.accept_low_coverage = accept_low_coverage;
    const float c3[3] = {click.x, click.y, click.z};
    return run_all_scans(all, bag_path, topic, yaml_path, out_path, solver, device, have_click ? c3 : nullptr,
                         have_click ? ILCC_SEED_CLICK : (auto_seed ? ILCC_SEED_AUTO : ILCC_SEED_AUTO_PLANAR));
  }
  myPointCloudPtr cloud(new myPointCloud);
  if (!bag_path.empty()) {   // get_lidar_corners.cpp:136-164
    uint32_t n = 0;
    int32_t st = ilcc_bag_first_cloud(device < 0 ? 0 : device, bag_path.c_str(), topic.c_str(), nullptr, 0, &n);
    if (st == ILCC_CAPACITY || st == ILCC_OK) {
      cloud->resize(n);
      st = ilcc_bag_first_cloud(device < 0 ? 0 : device, bag_path.c_str(), topic.c_str(),
                                reinterpret_cast<float*>(cloud->data()), n, &n);
    }
    if (st != ILCC_OK) {
      std::fprintf(stderr, "can't read lidar topic: %s\n", ilcc_last_error(nullptr));   // :157-161
      return 1;
    }
  } else {
    std::ifstream in(cloud_path, std::ios::binary | std::ios::ate);
    if (!in.is_open()) {
      std::fprintf(stderr, "can not open %s\n", cloud_path.c_str());
      return 1;
    }
    const std::streamsize bytes = in.tellg();
    in.seekg(0);
    cloud->resize((size_t)bytes / sizeof(PointXYZI));
    in.read(reinterpret_cast<char*>(cloud->data()), (std::streamsize)(cloud->size() * sizeof(PointXYZI)));
  }

  LidarCornersEst est(device, (uint32_t)cloud->size() + 1, (auto_seed || auto_planar) ? 4u : 1u);
  est.params().solver = (solver == "reference") ? ILCC_SOLVER_REFERENCE_LOCAL : ILCC_SOLVER_GRID;
  est.accept_ambiguous = accept_ambiguous;
  est.accept_low_coverage = accept_low_coverage;
  est.register_viewer();
  if (!yaml_path.empty() && !est.set_chessboard_param(yaml_path)) return 1;

  if (auto_seed || auto_planar) {
    if (!(auto_planar ? est.find_board_planar(cloud) : est.find_board(cloud))) {
      std::printf("no chessboard found\n");
      return 3;
    }
    std::printf("seed %.9g %.9g %.9g\n", est.m_click_point.x, est.m_click_point.y, est.m_click_point.z);
  } else {
    est.setROI(cloud, click);                        // get_lidar_corners.cpp:183
  }
  if (!est.EuclideanCluster()) return 3;             // :188
  est.PCA();                                         // :191
  std::vector<std::array<double, 3>> lidar_corner;
  if (!est.get_corners(lidar_corner)) return 4;      // :194
  std::cout << "add_corner" << std::endl;            // :196
  if (!save_corners2txt(est.m_cloud_corners, out_path)) {   // :197-198
    std::fprintf(stderr, "can not write %s\n", out_path.c_str());
    return 1;
  }
  const ilcc_result& r = est.result();
  std::printf("theta_t %.6f %.6f %.6f phase %d cost %.6f margin %.3f status %d corners %d -> %s\n", r.theta_t[0], r.theta_t[1],
              r.theta_t[2], r.phase, r.sel_cost, r.basin_margin, r.status, r.n_corners, out_path.c_str());
  return 0;
}
