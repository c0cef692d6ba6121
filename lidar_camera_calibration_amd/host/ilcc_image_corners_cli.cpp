// ilcc_image_corners -- ROS-free counterpart of get_image_corners_bag plus the MATLAB step, for machines
// without ROS, OpenCV or MATLAB (the GPU box): the first sensor_msgs/Image of a bag -> mono8 -> undistorted
// with the yaml's K and d -> chessboard corners -> `<camera><i>.txt` as ilcc_calib_lidar_cam reads it.
//   ilcc_image_corners --bag 20181101_1.bag --topic /camera/image_raw --yaml pointgrey.yaml --out pointgrey1.txt
//                      [--pgm undistorted.pgm] [--jpg-out <camera><i>.jpg] [--quality 95] [--device N]
//   ilcc_image_corners --jpg pointgrey1.jpg [--yaml pointgrey.yaml] [--board 7x5] --out pointgrey1.txt [--device N]
//   ilcc_image_corners --bag ... --topic ... --yaml ... --out pointgrey1.txt --all-images [--first N] [--stride N] [--max-images N]
//                      [--gate PX] [--report FILE] [--decode-threads N] [--huffman host|gpu] [--structure host|gpu]
//                      [--jpg-out-all PREFIX] [--quality 95]
// --all-images reads EVERY sensor_msgs/Image of the topic (include/ilcc_image_sequence.h): the boards of the images that hold one
// are fused into ONE board, written in the same format; --report writes one line per image.  It takes no --jpg, --jpg-out or --pgm.
// A topic that carries no sensor_msgs/Image but sensor_msgs/CompressedImage goes through include/ilcc_jpeg_sequence.h instead
// (the same output); --decode-threads is the number of host threads its Huffman decode runs on (0: 8, at most 16), and
// --huffman gpu decodes the scans on the device instead (K16, include/ilcc_jpeg_huffman.h; the threads then only prepare them).
// --structure gpu recovers every image's board on the device (K18, include/ilcc_image_structure.h) instead of a host thread: the
// same boards, the same files.
// --jpg-out-all PREFIX (with --all-images) writes every selected image, undistorted, as PREFIX<message index, 6 digits>.jpg
// (include/ilcc_jpeg_write_sequence.h: each file is what --jpg-out writes for that message alone); the Huffman coding runs on the
// device (K17) unless --huffman host is given.  With it --out may be left out: the corners are then not searched.
// --jpg takes the image from a JPEG file instead (libcbdetect/demo_all_pic.m:8-19 on one file).  Without --yaml the file
// is taken as already undistorted, as the reference's process_data/<camera><i>.jpg are, and the board is --board's
// (corners along x by corners along y, 7x5 when not given); with it, both come from the yaml as for a bag.
// --pgm writes the undistorted image as a binary PGM (P5).  --jpg-out writes it as the reference's imwrite does
// (get_image_corners_bag.cpp:104-110: process_data/<camera><i>.jpg, libjpeg at quality 95; include/ilcc_jpeg_write.h);
// with it --out may be left out, which is get_image_corners_bag alone: the corners are then not searched.
// Mirrors the per-bag body of /root/reference/ilcc2/test/get_image_corners_bag.cpp:67-112 and
// libcbdetect's findCorners / chessboardsFromCorners / plotChessboards dump.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ilcc_camera_image.h"
#include "ilcc_hip.h"
#include "ilcc_image_corners.h"
#include "ilcc_image_sequence.h"
#include "ilcc_jpeg.h"
#include "ilcc_jpeg_sequence.h"
#include "ilcc_jpeg_write.h"
#include "ilcc_jpeg_write_sequence.h"
#include "ilcc_sequence.h"

namespace {

const char* kUsage =
    "usage: ilcc_image_corners --bag file.bag --topic /camera/image_raw --yaml camera.yaml --out <camera><i>.txt "
    "[--pgm undistorted.pgm] [--jpg-out <camera><i>.jpg] [--quality 95] [--device N]\n"
    "       ilcc_image_corners --jpg file.jpg [--yaml camera.yaml] [--board 7x5] --out <camera><i>.txt [--device N]\n"
    "       ilcc_image_corners --bag file.bag --topic /camera/image_raw --yaml camera.yaml --out <camera><i>.txt --all-images "
    "[--first N] [--stride N] [--max-images N] [--gate PX] [--report FILE] [--decode-threads N] [--huffman host|gpu] "
    "[--structure host|gpu] [--jpg-out-all PREFIX] [--quality 95] [--device N]\n";

// true when the topic carries no sensor_msgs/Image but sensor_msgs/CompressedImage
bool compressed_only(const std::string& bag_path, const std::string& topic) {
  ilcc_bag_topic* it = nullptr;
  const bool raw = ilcc_bag_topic_open(bag_path.c_str(), topic.c_str(), "060021388200f6f0f447d0fcd9c64743", &it) == ILCC_OK;
  ilcc_bag_topic_close(it);
  if (raw) return false;
  it = nullptr;
  const bool compressed = ilcc_bag_topic_open(bag_path.c_str(), topic.c_str(), "8f7a12909da2c9d3332d540a0977563f", &it) == ILCC_OK;
  ilcc_bag_topic_close(it);
  return compressed;
}

// --all-images: every image of the topic, the fused board into out_path
int run_all_images(int device, const std::string& bag_path, const std::string& topic, const ilcc_camera_model& cam, int32_t board_w, int32_t board_h,
                   const ilcc_image_sequence_params& sp, uint32_t decode_threads, uint32_t huffman, const std::string& out_path,
                   const std::string& report) {
  ilcc_image_sequence_result r;
  std::vector<ilcc_image_record> images(1);
  ilcc_jpeg_sequence_params jp;
  ilcc_default_jpeg_sequence_params(&jp);
  jp.seq = sp;
  jp.decode_threads = decode_threads;
  jp.reserved0 = huffman;   // the route of the Huffman decode: 0 the host pool, 1 K16
  const bool compressed = compressed_only(bag_path, topic);
  auto run = [&](uint32_t cap) {
    return compressed ? ilcc_bag_corners_all_compressed_images(device, bag_path.c_str(), topic.c_str(), &cam, board_w, board_h, &jp, &r, images.data(), cap)
                      : ilcc_bag_corners_all_images(device, bag_path.c_str(), topic.c_str(), &cam, board_w, board_h, &sp, &r, images.data(), cap);
  };
  // one record is too few for most bags: the refusal says how many are needed, and nothing has run
  int32_t st = run(1);
  if (st == ILCC_CAPACITY && r.n_images > 1) {
    images.resize((size_t)r.n_images);
    st = run((uint32_t)images.size());
  }
  if (st != ILCC_OK && st != ILCC_AMBIGUOUS && st != ILCC_BOARD_NOT_FOUND) {
    std::fprintf(stderr, "all images: %s: %s\n", ilcc_strerror(st), ilcc_last_error(nullptr));
    return 1;
  }
  if (!report.empty()) {
    std::FILE* f = std::fopen(report.c_str(), "w");
    if (!f) {
      std::fprintf(stderr, "can not write %s\n", report.c_str());
      return 1;
    }
    for (int32_t k = 0; k < r.n_images; ++k)
      std::fprintf(f, "image %d message %u stamp %u.%09u status %d accepted %d used %d distance_px %.3f\n", k, images[k].message, images[k].stamp_sec,
                   images[k].stamp_nsec, images[k].status, images[k].accepted, images[k].used, images[k].distance < 0 ? -1.0 : images[k].distance);
    std::fclose(f);
  }
  int rc = st == ILCC_OK ? 0 : 4;
  if (st == ILCC_OK && ilcc_save_cam_corners(out_path.c_str(), r.rows, r.cols, r.xy) != ILCC_OK) {
    std::fprintf(stderr, "can not write %s\n", out_path.c_str());
    rc = 1;
  }
  if (st != ILCC_OK) std::fprintf(stderr, "no chessboard: %s\n", ilcc_last_error(nullptr));
  std::printf("all images: status %d images %d accepted %d used %d batches %d gate_px %.3f spread_rms_px %.3f spread_max_px %.3f ref_image %d board %d x %d -> %s\n",
              st, r.n_images, r.n_ok, r.n_used, r.n_batches, r.gate, r.spread_rms, r.spread_max, r.ref_image, r.rows, r.cols,
              st == ILCC_OK && rc == 0 ? out_path.c_str() : "-");
  return rc;
}

// --jpg-out-all: every selected image of the topic, undistorted, as <prefix><message index>.jpg
int run_save_all(int device, const std::string& bag_path, const std::string& topic, const ilcc_camera_model& cam, const ilcc_image_sequence_params& sp,
                 uint32_t route, int quality, const std::string& prefix) {
  ilcc_jpeg_write_sequence_params wp;
  ilcc_default_jpeg_write_sequence_params(&wp);
  wp.first = sp.first;
  wp.stride = sp.stride;
  wp.max_images = sp.max_images;
  wp.staging_bytes = sp.staging_bytes;
  wp.device_bytes = sp.device_bytes;
  wp.route = route;
  ilcc_jpeg_write_sequence_result r;
  const int32_t st = ilcc_bag_save_jpeg_all(device, bag_path.c_str(), topic.c_str(), &cam, prefix.c_str(), quality, &wp, &r, nullptr, 0);
  if (st != ILCC_OK) {
    std::fprintf(stderr, "can't write %s*.jpg: %s: %s\n", prefix.c_str(), ilcc_strerror(st), ilcc_last_error(nullptr));
    return 1;
  }
  std::printf("all images: %d files %llu bytes batches %d host_encoded %d -> %s*.jpg\n", r.n_images, (unsigned long long)r.file_bytes, r.n_batches,
              r.n_host_encoded, prefix.c_str());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  std::string bag_path, topic, yaml_path, out_path, pgm_path, jpg_path, jpg_out_path, jpg_out_all, report;
  int device = 0, quality = 95;
  bool all_images = false, sequence_option = false, huffman_given = false;
  uint32_t decode_threads = 0, huffman = 0;
  ilcc_image_sequence_params sp;
  ilcc_default_image_sequence_params(&sp);
  int32_t board_w = 7, board_h = 5;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--bag" && i + 1 < argc) bag_path = argv[++i];
    else if (a == "--topic" && i + 1 < argc) topic = argv[++i];
    else if (a == "--jpg" && i + 1 < argc) jpg_path = argv[++i];
    else if (a == "--board" && i + 1 < argc && std::sscanf(argv[i + 1], "%dx%d", &board_w, &board_h) == 2) ++i;
    else if (a == "--yaml" && i + 1 < argc) yaml_path = argv[++i];
    else if (a == "--out" && i + 1 < argc) out_path = argv[++i];
    else if (a == "--pgm" && i + 1 < argc) pgm_path = argv[++i];
    else if (a == "--jpg-out" && i + 1 < argc) jpg_out_path = argv[++i];
    else if (a == "--jpg-out-all" && i + 1 < argc) { jpg_out_all = argv[++i]; sequence_option = true; }
    else if (a == "--quality" && i + 1 < argc) quality = std::atoi(argv[++i]);
    else if (a == "--device" && i + 1 < argc) device = std::atoi(argv[++i]);
    else if (a == "--all-images") all_images = true;
    else if (a == "--first" && i + 1 < argc) { sp.first = (uint32_t)std::strtoul(argv[++i], nullptr, 10); sequence_option = true; }
    else if (a == "--stride" && i + 1 < argc) { sp.stride = (uint32_t)std::strtoul(argv[++i], nullptr, 10); sequence_option = true; }
    else if (a == "--max-images" && i + 1 < argc) { sp.max_images = (uint32_t)std::strtoul(argv[++i], nullptr, 10); sequence_option = true; }
    else if (a == "--gate" && i + 1 < argc) { sp.gate_px = std::atof(argv[++i]); sequence_option = true; }
    else if (a == "--report" && i + 1 < argc) { report = argv[++i]; sequence_option = true; }
    else if (a == "--decode-threads" && i + 1 < argc) { decode_threads = (uint32_t)std::strtoul(argv[++i], nullptr, 10); sequence_option = true; }
    else if (a == "--huffman" && i + 1 < argc && (std::string(argv[i + 1]) == "host" || std::string(argv[i + 1]) == "gpu")) {
      huffman = std::string(argv[++i]) == "gpu" ? 1u : 0u;
      sequence_option = huffman_given = true;
    } else if (a == "--structure" && i + 1 < argc && (std::string(argv[i + 1]) == "host" || std::string(argv[i + 1]) == "gpu")) {
      sp.reserved0 = std::string(argv[++i]) == "gpu" ? 1u : 0u;   // the route of structure recovery: 0 the host thread, 1 K18
      sequence_option = true;
    } else {
      std::fprintf(stderr, "unknown or incomplete argument: %s\n", a.c_str());
      return 2;
    }
  }
  const bool from_jpg = !jpg_path.empty();
  const bool bag_ok = !bag_path.empty() && !topic.empty() && !yaml_path.empty();
  const bool jpg_ok = bag_path.empty() && topic.empty() && pgm_path.empty() && jpg_out_path.empty();
  if ((out_path.empty() && (from_jpg || (jpg_out_path.empty() && jpg_out_all.empty()))) || (from_jpg ? !jpg_ok : !bag_ok)) {
    std::fprintf(stderr, "%s", kUsage);
    return 2;
  }
  if (all_images ? (from_jpg || !jpg_out_path.empty() || !pgm_path.empty() || (out_path.empty() && jpg_out_all.empty())) : sequence_option) {
    std::fprintf(stderr, "%s--all-images takes a bag and --out, no --jpg, --jpg-out or --pgm; --first, --stride, --max-images, --gate, --report, --structure, --decode-threads and --huffman need it, and so does --jpg-out-all, with which --out may be left out\n", kUsage);
    return 2;
  }
  ilcc_camera_model cam{};
  if (!yaml_path.empty()) {
    if (ilcc_read_camera_yaml(yaml_path.c_str(), &cam) != ILCC_OK) {
      std::fprintf(stderr, "%s\n", ilcc_last_error(nullptr));   // "can not open ..." as ImageCornersEst.cpp:20-24
      return 1;
    }
    // the board: corner_in_x x corner_in_y of the same yaml (ilcc_set_chessboard_param stores them + 1, smaller first)
    ilcc_params params;
    ilcc_default_params(&params);
    if (ilcc_set_chessboard_param(&params, yaml_path.c_str()) != ILCC_OK) {
      std::fprintf(stderr, "%s\n", ilcc_last_error(nullptr));
      return 1;
    }
    board_w = params.board_h - 1;
    board_h = params.board_w - 1;
  }
  if (board_w < 3 || board_h < 3) {
    std::fprintf(stderr, "the board needs at least 3 x 3 corners\n");
    return 2;
  }

  if (all_images && !jpg_out_all.empty()) {   // the files are coded on the device unless --huffman host says otherwise
    const int rc = run_save_all(device, bag_path, topic, cam, sp, huffman_given && huffman == 0 ? 1u : 0u, quality, jpg_out_all);
    if (rc != 0 || out_path.empty()) return rc;
  }
  if (all_images) return run_all_images(device, bag_path, topic, cam, board_w, board_h, sp, decode_threads, huffman, out_path, report);

  if (!pgm_path.empty()) {
    int32_t w = 0, h = 0;
    int32_t st = ilcc_bag_first_image(device, bag_path.c_str(), topic.c_str(), &cam, nullptr, 0, &w, &h);
    std::vector<uint8_t> pixels;
    if (st == ILCC_CAPACITY || st == ILCC_OK) {
      pixels.resize((size_t)w * (size_t)h);
      st = ilcc_bag_first_image(device, bag_path.c_str(), topic.c_str(), &cam, pixels.data(), pixels.size(), &w, &h);
    }
    if (st != ILCC_OK) {
      std::fprintf(stderr, "can't read image topic: %s\n", ilcc_last_error(nullptr));
      return 1;
    }
    FILE* f = std::fopen(pgm_path.c_str(), "wb");
    bool ok = f != nullptr;
    if (f) {
      ok = std::fprintf(f, "P5\n%d %d\n255\n", w, h) > 0 && std::fwrite(pixels.data(), 1, pixels.size(), f) == pixels.size();
      ok = (std::fclose(f) == 0) && ok;
    }
    if (!ok) {
      std::fprintf(stderr, "can not write %s\n", pgm_path.c_str());
      return 1;
    }
  }

  if (!jpg_out_path.empty()) {
    if (ilcc_bag_save_jpeg(device, bag_path.c_str(), topic.c_str(), &cam, jpg_out_path.c_str(), quality) != ILCC_OK) {
      std::fprintf(stderr, "can't write %s: %s\n", jpg_out_path.c_str(), ilcc_last_error(nullptr));
      return 1;
    }
    if (out_path.empty()) {
      std::printf("image %d x %d -> %s\n", cam.width, cam.height, jpg_out_path.c_str());
      return 0;
    }
  }

  int32_t rows = 0, cols = 0;
  std::vector<double> xy((size_t)board_w * board_h * 2);
  const int32_t st = from_jpg ? ilcc_jpeg_find_chessboard(device, jpg_path.c_str(), yaml_path.empty() ? nullptr : &cam, board_w, board_h,
                                                          &rows, &cols, xy.data())
                              : ilcc_bag_find_chessboard(device, bag_path.c_str(), topic.c_str(), &cam, board_w, board_h, &rows, &cols,
                                                         xy.data());
  if (st == ILCC_BOARD_NOT_FOUND || st == ILCC_AMBIGUOUS) {
    std::fprintf(stderr, "no chessboard: %s\n", ilcc_last_error(nullptr));
    return 4;
  }
  if (st != ILCC_OK) {
    std::fprintf(stderr, "%s: %s\n", from_jpg ? "can't read image file" : "can't read image topic", ilcc_last_error(nullptr));
    return 1;
  }
  if (ilcc_save_cam_corners(out_path.c_str(), rows, cols, xy.data()) != ILCC_OK) {
    std::fprintf(stderr, "can not write %s\n", out_path.c_str());
    return 1;
  }
  if (from_jpg) std::printf("%s board %d x %d -> %s\n", jpg_path.c_str(), rows, cols, out_path.c_str());
  else std::printf("image %d x %d board %d x %d -> %s\n", cam.width, cam.height, rows, cols, out_path.c_str());
  return 0;
}
