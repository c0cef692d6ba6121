// Stand-alone check of csrc/sequence_host.cpp (ilcc_fuse_corners) for tests/test_sequence_cpu.py, built with ASan and UBSan:
// reads constructed cases with the restatement's answers (hex floats), runs the fusion, and exits 1 on the first mismatch.
//   cases.txt: <n_cases>, then per case
//     <name> <n> <a> <b> <gate>
//     accepted[n]
//     corners[n a b 3]
//     <status> <n_ok> <n_used> <ref_scan> <n_corners> <spread_max> <spread_rms>
//     used[n]
//     corners[n_corners 3]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "ilcc_sequence.h"

static double number(std::istream& in) {
  std::string t;
  in >> t;
  return std::strtod(t.c_str(), nullptr);   // hex floats and "nan"
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in.is_open()) return 2;
  int n_cases = 0;
  in >> n_cases;
  for (int k = 0; k < n_cases; ++k) {
    std::string name;
    uint32_t n = 0, a = 0, b = 0;
    in >> name >> n >> a >> b;
    const double gate = number(in);
    std::vector<uint8_t> accepted(n), used(n), want_used(n);
    std::vector<double> dist(n);
    for (uint32_t i = 0; i < n; ++i) {
      int v;
      in >> v;
      accepted[i] = (uint8_t)v;
    }
    std::vector<float> corners((size_t)n * a * b * 3);   // exactly sized: a read past a scan is an ASan report
    for (float& v : corners) v = (float)number(in);
    int status, n_ok, n_used, ref_scan, n_corners;
    in >> status >> n_ok >> n_used >> ref_scan >> n_corners;
    const double spread_max = number(in), spread_rms = number(in);
    for (uint32_t i = 0; i < n; ++i) {
      int v;
      in >> v;
      want_used[i] = (uint8_t)v;
    }
    std::vector<float> want((size_t)n_corners * 3);
    for (float& v : want) v = (float)number(in);
    if (!in) {
      std::printf("case %d: cannot parse\n", k);
      return 2;
    }
    ilcc_fused_corners out;
    const int32_t st = ilcc_fuse_corners(corners.data(), accepted.data(), n, a, b, gate, &out, used.data(), dist.data());
    bool ok = st == status && out.status == status && out.n_scans == (int)n && out.n_ok == n_ok && out.n_used == n_used && out.ref_scan == ref_scan &&
              out.n_corners == n_corners && out.spread_max == spread_max && std::fabs(out.spread_rms - spread_rms) <= 1e-12 * std::fabs(spread_rms);
    ok = ok && (n == 0 || std::memcmp(used.data(), want_used.data(), n) == 0);
    ok = ok && (want.empty() || std::memcmp(out.corners, want.data(), 4 * want.size()) == 0);
    // the optional outputs are optional
    ilcc_fused_corners again;
    ok = ok && ilcc_fuse_corners(corners.data(), accepted.data(), n, a, b, gate, &again, nullptr, nullptr) == st &&
         std::memcmp(&again, &out, sizeof(out)) == 0;
    if (!ok) {
      std::printf("mismatch in case %s: status %d/%d ok %d/%d used %d/%d ref %d/%d corners %d/%d max %a/%a rms %a/%a\n", name.c_str(), st, status, out.n_ok,
                  n_ok, out.n_used, n_used, out.ref_scan, ref_scan, out.n_corners, n_corners, out.spread_max, spread_max, out.spread_rms, spread_rms);
      return 1;
    }
  }
  std::printf("cases %d ok\n", n_cases);
  return 0;
}
