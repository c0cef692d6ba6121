// Stand-alone check of csrc/paired_host.cpp (ilcc_pair_by_stamp, ilcc_save_pcd_xyzrgb) and csrc/paired_cut.cpp (the batch cut of
// the paired chains), built by tests/test_paired_cpu.py with -fsanitize=address,undefined: no GPU, no library, no python.
//   paired_host_check cases.txt out_dir [cut_cases.txt]
// cases.txt: the number of cases, then per case: "n_clouds n_images max_dt", the cloud stamps, the image stamps, the expected
// image_of, the expected dt_ns (a line each, possibly empty).  Prints "mismatch ..." and exits 1 when an answer differs.
// Then writes out_dir/pcd_<n>.pcd for n = 0, 1, 1000 (record k: floats k, -(k + 1), k / 2 and the rgb bits 0x00010203 * (k % 7)), and
// reports the statuses of the refusals.
// cut_cases.txt: the number of cases, then per case: "n_scans n_images bgr_bytes staging image device per_member member_cap
// stage_unpaired", the scans' data_bytes, points and pair, the images' raw bytes (a line each), "status n_batches", and for status 0
// per batch "first_scan scans blob_bytes points raw_bytes bgr_bytes", its members, its images as (image raw_at bgr_at) triples, then
// the largest "members blob_bytes points raw_bytes bgr_bytes".  Every batch is printed; "mismatch in cut case ..." and exit 1 when
// the status, a batch or the largest differs.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ilcc_paired.h"
#include "paired_cut.h"

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

// 0: every case equals its expectation; 1: a mismatch (printed); 2: the file is not what the header comment says
static int check_cuts(const char* path) {
  std::ifstream in(path);
  if (!in) return 2;
  const std::vector<uint64_t> head = read_line<uint64_t>(in);
  if (head.size() != 1) return 2;
  for (uint64_t k = 0; k < head[0]; ++k) {
    const std::vector<uint64_t> dims = read_line<uint64_t>(in);
    if (dims.size() != 9) return 2;
    const std::vector<uint64_t> data = read_line<uint64_t>(in), points = read_line<uint64_t>(in);
    const std::vector<int64_t> pair = read_line<int64_t>(in);
    const std::vector<uint64_t> raw = read_line<uint64_t>(in);   // exact-size heap copy: an image index past its end is AddressSanitizer's to report
    const std::vector<int64_t> want = read_line<int64_t>(in);
    if (data.size() != dims[0] || points.size() != dims[0] || pair.size() != dims[0] || raw.size() != dims[1] || want.size() != 2) return 2;
    std::vector<ilcc::PairedScan> scans(dims[0]);
    for (uint64_t s = 0; s < dims[0]; ++s) scans[s] = ilcc::PairedScan{data[s], points[s], pair[s]};
    ilcc::PairedBudgets budgets;
    budgets.staging = dims[3];
    budgets.image = dims[4];
    budgets.device = dims[5];
    budgets.per_member = dims[6];
    budgets.member_cap = (uint32_t)dims[7];
    budgets.stage_unpaired = dims[8] != 0;
    std::vector<ilcc::PairedBatch> batches;
    ilcc::PairedLargest largest;
    std::string why;
    const int32_t st = ilcc::paired_cut(scans.data(), (uint32_t)scans.size(), raw.data(), dims[2], budgets, &batches, &largest, &why);
    bool same = st == want[0] && (st != ILCC_OK || batches.size() == (uint64_t)want[1]) && (st == ILCC_OK) == why.empty();
    for (size_t b = 0; st == ILCC_OK && b < batches.size(); ++b) {
      const ilcc::PairedBatch& B = batches[b];
      std::printf("cut case %" PRIu64 " batch %zu: first_scan %u scans %u members %zu blob %" PRIu64 " points %" PRIu64 " raw %" PRIu64 " bgr %" PRIu64
                  " images %zu\n", k, b, B.first_scan, B.scans, B.members.size(), B.blob_bytes, B.points, B.raw_bytes, B.bgr_bytes, B.images.size());
      if (!same) continue;   // fewer batches expected than made: no lines to read them from
      const std::vector<uint64_t> row = read_line<uint64_t>(in), members = read_line<uint64_t>(in), images = read_line<uint64_t>(in);
      std::vector<uint64_t> got_images;
      for (const ilcc::ImageSlot& slot : B.images) got_images.insert(got_images.end(), {(uint64_t)slot.image, slot.raw_at, slot.bgr_at});
      same = row == std::vector<uint64_t>{B.first_scan, B.scans, B.blob_bytes, B.points, B.raw_bytes, B.bgr_bytes} &&
             members == std::vector<uint64_t>(B.members.begin(), B.members.end()) && images == got_images;
    }
    if (same && st == ILCC_OK)
      same = read_line<uint64_t>(in) == std::vector<uint64_t>{largest.members, largest.blob_bytes, largest.points, largest.raw_bytes, largest.bgr_bytes};
    if (!same) {
      std::printf("mismatch in cut case %" PRIu64 " (status %d %s)\n", k, st, why.c_str());
      return 1;
    }
  }
  std::printf("cut cases %" PRIu64 " ok\n", head[0]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) {
    std::fprintf(stderr, "usage: paired_host_check cases.txt out_dir [cut_cases.txt]\n");
    return 2;
  }
  if (argc == 4) {
    const int cuts = check_cuts(argv[3]);
    if (cuts != 0) return cuts;
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
