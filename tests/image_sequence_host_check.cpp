// Stand-alone driver of csrc/image_sequence_host.cpp for tests/test_image_sequence_cpu.py: built with the fusion ALONE under
// AddressSanitizer and UBSan.  Reads constructed cases with the restatement's answer beside them (hex doubles), runs
// ilcc_fuse_image_corners and ilcc_image_sequence_cut, compares exactly, exits 1 on the first mismatch.
//
//   file:  <n_cases>
//   case:  <name> <n> <a> <b> <gate hex>
//          <accepted ...>            (n flags; "-" when n == 0)
//          <rows ...> / <cols ...>   (n each; "-" when n == 0)
//          <xy ...>                  (n * a * b * 2 hex doubles or nan; "-" when empty)
//          <status> <n_ok> <n_used> <ref_image> <rows> <cols> <gate hex> <spread_max hex> <spread_rms hex>
//          <used ...> / <dist ...>   (n each; "-" when n == 0)
//          <fused xy ...>            (rows * cols * 2 hex doubles when status == 0, else "-")
//   then:  cut <n> <per_image> <staging> <device> / <raw ...> / <status> <firsts ...>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ilcc_image_sequence.h"

static std::vector<std::string> words(std::istream& in) {
  std::string line;
  std::getline(in, line);
  std::istringstream ss(line);
  std::vector<std::string> out;
  for (std::string w; ss >> w;)
    if (w != "-") out.push_back(w);
  return out;
}

static double num(const std::string& s) { return s == "nan" ? std::nan("") : std::strtod(s.c_str(), nullptr); }

static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0 || a == b; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  int n_cases = std::atoi(words(in).at(0).c_str());
  for (int k = 0; k < n_cases; ++k) {
    const auto head = words(in);
    const std::string name = head.at(0);
    const uint32_t n = (uint32_t)std::atoi(head.at(1).c_str()), a = (uint32_t)std::atoi(head.at(2).c_str()), b = (uint32_t)std::atoi(head.at(3).c_str());
    const double gate = num(head.at(4));
    std::vector<uint8_t> accepted;
    for (auto& w : words(in)) accepted.push_back((uint8_t)std::atoi(w.c_str()));
    std::vector<int32_t> rows, cols;
    for (auto& w : words(in)) rows.push_back(std::atoi(w.c_str()));
    for (auto& w : words(in)) cols.push_back(std::atoi(w.c_str()));
    std::vector<double> xy;   // exactly n * a * b * 2: a read past it is ASan's to find
    for (auto& w : words(in)) xy.push_back(num(w));
    const auto want = words(in);
    std::vector<uint8_t> want_used;
    for (auto& w : words(in)) want_used.push_back((uint8_t)std::atoi(w.c_str()));
    std::vector<double> want_dist, want_xy;
    for (auto& w : words(in)) want_dist.push_back(num(w));
    for (auto& w : words(in)) want_xy.push_back(num(w));
    if (accepted.size() != n || rows.size() != n || cols.size() != n || xy.size() != (size_t)n * a * b * 2) {
      std::printf("case %s: malformed\n", name.c_str());
      return 2;
    }
    ilcc_fused_image_corners out;
    std::vector<uint8_t> used(n);
    std::vector<double> dist(n);
    const int32_t st = ilcc_fuse_image_corners(xy.data(), rows.data(), cols.data(), accepted.data(), n, a, b, gate, &out, used.data(), dist.data());
    bool ok = st == out.status && st == std::atoi(want.at(0).c_str()) && out.n_images == (int32_t)n && out.n_ok == std::atoi(want.at(1).c_str()) &&
              out.n_used == std::atoi(want.at(2).c_str()) && out.ref_image == std::atoi(want.at(3).c_str()) && out.rows == std::atoi(want.at(4).c_str()) &&
              out.cols == std::atoi(want.at(5).c_str()) && same(out.gate, num(want.at(6))) && same(out.spread_max, num(want.at(7))) &&
              same(out.spread_rms, num(want.at(8)));
    if (st != ILCC_BAD_ARGUMENT)
      for (uint32_t i = 0; i < n && ok; ++i) ok = used[i] == want_used.at(i) && same(dist[i], want_dist.at(i));
    for (size_t i = 0; i < want_xy.size() && ok; ++i) ok = same(out.xy[i], want_xy[i]);
    if (st != ILCC_OK)
      for (size_t i = 0; i < sizeof(out.xy) / sizeof(double) && ok; ++i) ok = out.xy[i] == 0.0;
    if (!ok) {
      std::printf("case %s: mismatch (status %d, n_ok %d, n_used %d, ref %d, %d x %d, gate %a, max %a, rms %a)\n", name.c_str(), st, out.n_ok, out.n_used,
                  out.ref_image, out.rows, out.cols, out.gate, out.spread_max, out.spread_rms);
      return 1;
    }
  }
  int n_cuts = 0;
  for (;;) {
    const auto head = words(in);
    if (head.empty() || head[0] != "cut") break;
    const uint32_t n = (uint32_t)std::atoi(head.at(1).c_str());
    std::vector<uint64_t> raw;
    for (auto& w : words(in)) raw.push_back(std::strtoull(w.c_str(), nullptr, 10));
    const auto want = words(in);
    std::vector<uint32_t> firsts(n + 1);   // exactly n + 1
    uint32_t nb = 0;
    const int32_t st = ilcc_image_sequence_cut(raw.data(), n, std::strtoull(head.at(2).c_str(), nullptr, 10), std::strtoull(head.at(3).c_str(), nullptr, 10),
                                               std::strtoull(head.at(4).c_str(), nullptr, 10), firsts.data(), &nb);
    bool ok = raw.size() == n && st == std::atoi(want.at(0).c_str());
    if (ok && st == ILCC_OK) {
      ok = nb + 1 == want.size() - 1 || (n == 0 && nb == 0);
      for (uint32_t i = 0; ok && i + 1 < want.size(); ++i) ok = firsts[i] == (uint32_t)std::atoi(want[i + 1].c_str());
    }
    if (!ok) {
      std::printf("cut %d: mismatch (status %d, %u batches)\n", n_cuts, st, nb);
      return 1;
    }
    ++n_cuts;
  }
  std::printf("cases %d ok, cuts %d ok\n", n_cases, n_cuts);
  return 0;
}
