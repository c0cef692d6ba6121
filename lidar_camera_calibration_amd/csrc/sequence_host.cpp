// sequence_host.cpp -- ilcc_fuse_corners (include/ilcc_sequence.h): the per-scan corner sets of a recording -> one set.
// Plain C++ without HIP, fp64, built with -ffp-contract=off so that every sum below is the unfused IEEE one that
// tests/sequence_ref.py restates; it also builds alone, under sanitizers, for tests/test_sequence_cpu.py.
// Host work on purpose: a scan contributes 3 (board_w - 1) (board_h - 1) numbers (72 for the 7 x 5 board), hundreds of scans are
// kilobytes -- the argument that keeps libilcc_calib on the host.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ilcc_sequence.h"

namespace {

// index of corner c of the reference numbering in a scan numbered by `variant`
inline uint32_t variant_index(uint32_t c, uint32_t a, uint32_t b, int variant) {
  uint32_t i = c / b, j = c - i * b;
  if (variant & 1) i = a - 1 - i;
  if (variant & 2) j = b - 1 - j;
  return i * b + j;
}

// per-coordinate median of the rows listed in `scans` (aligned corners, C3 doubles per row)
void median_of(const std::vector<double>& aligned, const std::vector<uint32_t>& scans, uint32_t C3, std::vector<double>* out) {
  std::vector<double> v(scans.size());
  out->resize(C3);
  for (uint32_t k = 0; k < C3; ++k) {
    for (size_t s = 0; s < scans.size(); ++s) v[s] = aligned[(size_t)scans[s] * C3 + k];
    std::sort(v.begin(), v.end());
    const size_t m = v.size() / 2;
    (*out)[k] = (v.size() & 1) ? v[m] : (v[m - 1] + v[m]) / 2;
  }
}

// the largest squared corner distance of row `s` to m; *sum gets every corner's squared distance added
double max_d2(const std::vector<double>& aligned, uint32_t s, const double* m, uint32_t C, double* sum) {
  double worst = 0;
  for (uint32_t c = 0; c < C; ++c) {
    const double* p = &aligned[((size_t)s * C + c) * 3];
    const double dx = p[0] - m[3 * c], dy = p[1] - m[3 * c + 1], dz = p[2] - m[3 * c + 2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 > worst) worst = d2;
    if (sum) *sum += d2;
  }
  return worst;
}

int32_t fuse(const float* corners, const uint8_t* accepted, uint32_t n, uint32_t a, uint32_t b, double gate, ilcc_fused_corners* out,
             uint8_t* used_out, double* dist_out) {
  const uint32_t C = a * b, C3 = 3 * C;
  out->n_scans = (int32_t)n;
  if (used_out) std::memset(used_out, 0, n);
  if (dist_out)
    for (uint32_t i = 0; i < n; ++i) dist_out[i] = -1;
  std::vector<uint32_t> S;   // rows of `aligned` <-> input scans
  for (uint32_t i = 0; i < n; ++i)
    if (accepted[i]) S.push_back(i);
  out->n_ok = (int32_t)S.size();
  if (S.empty()) return ILCC_BOARD_NOT_FOUND;
  for (uint32_t s : S)
    for (uint32_t k = 0; k < C3; ++k)
      if (!std::isfinite(corners[(size_t)s * C3 + k])) return ILCC_BAD_ARGUMENT;
  out->ref_scan = (int32_t)S[0];

  // 2. alignment to the first accepted scan
  std::vector<double> aligned(S.size() * (size_t)C3);
  const float* ref = corners + (size_t)S[0] * C3;
  for (size_t r = 0; r < S.size(); ++r) {
    const float* scan = corners + (size_t)S[r] * C3;
    int best = 0;
    double best_cost = 0;
    for (int v = 0; v < 4; ++v) {
      double cost = 0;
      for (uint32_t c = 0; c < C; ++c) {
        const float* p = scan + 3 * variant_index(c, a, b, v);
        for (int k = 0; k < 3; ++k) {
          const double d = (double)p[k] - (double)ref[3 * c + k];
          cost += d * d;
        }
      }
      if (v == 0 || cost < best_cost) {
        best = v;
        best_cost = cost;
      }
    }
    for (uint32_t c = 0; c < C; ++c) {
      const float* p = scan + 3 * variant_index(c, a, b, best);
      for (int k = 0; k < 3; ++k) aligned[(r * C + c) * 3 + k] = (double)p[k];
    }
  }

  // 3.-5. one gating round against the median of all accepted scans
  std::vector<uint32_t> rows(S.size()), used;
  for (size_t r = 0; r < S.size(); ++r) rows[r] = (uint32_t)r;
  std::vector<double> m;
  median_of(aligned, rows, C3, &m);
  const double gate2 = gate * gate;
  std::vector<double> d2(S.size());
  for (size_t r = 0; r < S.size(); ++r) {
    d2[r] = max_d2(aligned, (uint32_t)r, m.data(), C, nullptr);
    if (d2[r] <= gate2) used.push_back((uint32_t)r);
  }
  out->n_used = (int32_t)used.size();
  if (used_out)
    for (uint32_t r : used) used_out[S[r]] = 1;
  if (used.empty() || 2 * used.size() <= S.size()) {
    if (dist_out)
      for (size_t r = 0; r < S.size(); ++r) dist_out[S[r]] = std::sqrt(d2[r]);
    return ILCC_AMBIGUOUS;
  }

  // 6. the median of the used scans, as fp32, and the spread around it
  median_of(aligned, used, C3, &m);
  for (uint32_t k = 0; k < C3; ++k) {
    out->corners[k] = (float)m[k];
    m[k] = (double)out->corners[k];
  }
  out->n_corners = (int32_t)C;
  double worst = 0, sum = 0;
  for (uint32_t r : used) {
    const double w = max_d2(aligned, r, m.data(), C, &sum);
    if (w > worst) worst = w;
  }
  out->spread_max = std::sqrt(worst);
  out->spread_rms = std::sqrt(sum / ((double)used.size() * (double)C));
  if (dist_out)
    for (size_t r = 0; r < S.size(); ++r) dist_out[S[r]] = std::sqrt(max_d2(aligned, (uint32_t)r, m.data(), C, nullptr));
  return ILCC_OK;
}

}  // namespace

extern "C" int32_t ilcc_fuse_corners(const float* corners, const uint8_t* accepted, uint32_t n, uint32_t a, uint32_t b, double gate,
                                     ilcc_fused_corners* out, uint8_t* used_out, double* dist_out) {
  if (!out) return ILCC_BAD_ARGUMENT;
  std::memset(out, 0, sizeof(*out));
  out->ref_scan = -1;
  int32_t st;
  if ((n && (!corners || !accepted)) || a < 1 || b < 1 || (uint64_t)a * b > ILCC_MAX_CORNERS || !(gate > 0) || !std::isfinite(gate)) {
    st = ILCC_BAD_ARGUMENT;
  } else {
    try {   // no exception crosses the C-ABI
      st = fuse(corners, accepted, n, a, b, gate, out, used_out, dist_out);
    } catch (...) {
      st = ILCC_IO_ERROR;
    }
  }
  out->status = st;
  return st;
}
