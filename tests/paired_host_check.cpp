// Stand-alone check of csrc/paired_host.cpp (ilcc_pair_by_stamp, ilcc_save_pcd_xyzrgb), built by tests/test_paired_cpu.py with
// -fsanitize=address,undefined: no GPU, no library, no python.
//   paired_host_check cases.txt out_dir
// cases.txt: the number of cases, then per case: "n_clouds n_images max_dt", the cloud stamps, the image stamps, the expected
// image_of, the expected dt_ns (a line each, possibly empty).  Prints "mismatch ..." and exits 1 when an answer differs.
// Then writes out_dir/pcd_<n>.pcd for n = 0, 1, 1000 (record k: floats k, -(k + 1), k / 2 and the rgb bits 0x00010203 * (k % 7)), and
// reports the statuses of the refusals.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ilcc_paired.h"

template <typename T>
static std::vector<T> read_line(std::ifstream& in) {
  std::string line;
  std::getline(in, line);
  std::istringstream ss(line);
  std::vector<T> out;
  T v;
  while (ss >> v) out.push_back(v);
  return out;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: paired_host_check cases.txt out_dir\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) return 2;
  const std::vector<uint64_t> head = read_line<uint64_t>(in);
  if (head.size() != 1) return 2;
  for (uint64_t k = 0; k < head[0]; ++k) {
    const std::vector<uint64_t> dims = read_line<uint64_t>(in);
    if (dims.size() != 3) return 2;
    const std::vector<uint64_t> clouds = read_line<uint64_t>(in), images = read_line<uint64_t>(in);
    const std::vector<int64_t> want_of = read_line<int64_t>(in), want_dt = read_line<int64_t>(in);
    if (clouds.size() != dims[0] || images.size() != dims[1] || want_of.size() != dims[0] || want_dt.size() != dims[0]) return 2;
    // exact-size heap copies: a read or write one past either end is AddressSanitizer's to report
    std::vector<int64_t> got_of(dims[0], 77), got_dt(dims[0], 77);
    const int32_t st = ilcc_pair_by_stamp(clouds.data(), dims[0], images.data(), dims[1], dims[2], got_of.data(), got_dt.data());
    if (st != ILCC_OK || got_of != want_of || got_dt != want_dt) {
      std::printf("mismatch in case %" PRIu64 " (status %d)\n", k, st);
      return 1;
    }
  }
  std::printf("cases %" PRIu64 " ok\n", head[0]);

  for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)1000}) {
    std::vector<float> rec(4 * n);
    for (uint64_t k = 0; k < n; ++k) {
      rec[4 * k] = (float)k;
      rec[4 * k + 1] = -(float)(k + 1);
      rec[4 * k + 2] = (float)k / 2;
      const uint32_t rgb = 0x00010203u * (uint32_t)(k % 7);
      std::memcpy(&rec[4 * k + 3], &rgb, 4);
    }
    const std::string path = std::string(argv[2]) + "/pcd_" + std::to_string(n) + ".pcd";
    if (ilcc_save_pcd_xyzrgb(path.c_str(), n ? rec.data() : nullptr, n) != ILCC_OK) {
      std::printf("mismatch: can not write %s\n", path.c_str());
      return 1;
    }
  }
  const std::string nowhere = std::string(argv[2]) + "/no_such_dir/a.pcd";
  float one[4] = {0, 0, 0, 0};
  uint64_t stamp = 1;
  int64_t out = 0;
  std::printf("unwritable %d null_name %d null_records %d null_clouds %d null_images %d\n", ilcc_save_pcd_xyzrgb(nowhere.c_str(), one, 1),
              ilcc_save_pcd_xyzrgb(nullptr, one, 1), ilcc_save_pcd_xyzrgb(nowhere.c_str(), nullptr, 1),
              ilcc_pair_by_stamp(nullptr, 1, &stamp, 1, 0, &out, &out), ilcc_pair_by_stamp(&stamp, 1, nullptr, 1, 0, &out, &out));
  return 0;
}
