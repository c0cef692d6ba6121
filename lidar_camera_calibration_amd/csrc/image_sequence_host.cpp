// image_sequence_host.cpp -- ilcc_fuse_image_corners and ilcc_image_sequence_cut (include/ilcc_image_sequence.h): the per-image
// boards of a recording -> one board, and the batches of a selection.  Plain C++ without HIP, fp64, built with -ffp-contract=off
// so that every sum below is the unfused IEEE one that tests/image_sequence_ref.py restates; it also builds alone, under
// sanitizers, for tests/test_image_sequence_cpu.py.  Host work on purpose: an image contributes 2 a b numbers (70 for the 7 x 5
// board), hundreds of images are kilobytes.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ilcc_image_sequence.h"

namespace {

constexpr uint64_t kDefaultStagingBytes = 256ull << 20, kDefaultDeviceBytes = 512ull << 20;

// index, in an image numbered by `variant`, of entry c = i C + j of the R x C reference numbering
inline uint32_t variant_index(uint32_t c, uint32_t R, uint32_t C, int variant) {
  uint32_t i = c / C, j = c - i * C;
  if (variant & 1) i = R - 1 - i;
  if (variant & 2) j = C - 1 - j;
  return (variant & 4) ? j * R + i : i * C + j;   // 4-7: the image is C x R, read at (j, i)
}

// per-coordinate median of the rows listed in `images` (aligned boards, K doubles per row)
void median_of(const std::vector<double>& aligned, const std::vector<uint32_t>& images, uint32_t K, std::vector<double>* out) {
  std::vector<double> v(images.size());
  out->resize(K);
  for (uint32_t k = 0; k < K; ++k) {
    for (size_t s = 0; s < images.size(); ++s) v[s] = aligned[(size_t)images[s] * K + k];
    std::sort(v.begin(), v.end());
    const size_t m = v.size() / 2;
    (*out)[k] = (v.size() & 1) ? v[m] : (v[m - 1] + v[m]) / 2;
  }
}

// the largest squared corner distance of row `s` to m; *sum gets every corner's squared distance added
double max_d2(const std::vector<double>& aligned, uint32_t s, const double* m, uint32_t N, double* sum) {
  double worst = 0;
  for (uint32_t c = 0; c < N; ++c) {
    const double* p = &aligned[((size_t)s * N + c) * 2];
    const double du = p[0] - m[2 * c], dv = p[1] - m[2 * c + 1];
    const double d2 = du * du + dv * dv;
    if (d2 > worst) worst = d2;
    if (sum) *sum += d2;
  }
  return worst;
}

int32_t fuse(const double* xy, const int32_t* rows, const int32_t* cols, const uint8_t* accepted, uint32_t n, uint32_t a, uint32_t b,
             double gate_px, ilcc_fused_image_corners* out, uint8_t* used_out, double* dist_out) {
  const uint32_t N = a * b, K = 2 * N;
  out->n_images = (int32_t)n;
  if (used_out) std::memset(used_out, 0, n);
  if (dist_out)
    for (uint32_t i = 0; i < n; ++i) dist_out[i] = -1;
  std::vector<uint32_t> S;   // rows of `aligned` <-> input images
  for (uint32_t i = 0; i < n; ++i)
    if (accepted[i]) S.push_back(i);
  out->n_ok = (int32_t)S.size();
  if (S.empty()) return ILCC_BOARD_NOT_FOUND;
  for (uint32_t s : S) {
    const bool ab = rows[s] == (int32_t)a && cols[s] == (int32_t)b, ba = rows[s] == (int32_t)b && cols[s] == (int32_t)a;
    if (!ab && !ba) return ILCC_BAD_ARGUMENT;
    for (uint32_t k = 0; k < K; ++k)
      if (!std::isfinite(xy[(size_t)s * K + k])) return ILCC_BAD_ARGUMENT;
  }
  out->ref_image = (int32_t)S[0];
  const uint32_t R = (uint32_t)rows[S[0]], C = (uint32_t)cols[S[0]];
  out->rows = (int32_t)R;
  out->cols = (int32_t)C;

  // 2. alignment to the first accepted image
  std::vector<double> aligned(S.size() * (size_t)K);
  const double* ref = xy + (size_t)S[0] * K;
  for (size_t r = 0; r < S.size(); ++r) {
    const double* img = xy + (size_t)S[r] * K;
    const bool same = (uint32_t)rows[S[r]] == R && (uint32_t)cols[S[r]] == C, transposed = (uint32_t)rows[S[r]] == C && (uint32_t)cols[S[r]] == R;
    int best = -1;
    double best_cost = 0;
    for (int v = 0; v < 8; ++v) {
      if (v < 4 ? !same : !transposed) continue;
      double cost = 0;
      for (uint32_t c = 0; c < N; ++c) {
        const double* p = img + 2 * variant_index(c, R, C, v);
        for (int k = 0; k < 2; ++k) {
          const double d = p[k] - ref[2 * c + k];
          cost += d * d;
        }
      }
      if (best < 0 || cost < best_cost) {
        best = v;
        best_cost = cost;
      }
    }
    for (uint32_t c = 0; c < N; ++c) {
      const double* p = img + 2 * variant_index(c, R, C, best);
      aligned[(r * N + c) * 2] = p[0];
      aligned[(r * N + c) * 2 + 1] = p[1];
    }
  }

  // 3.-5. one gating round against the median of all accepted images
  std::vector<uint32_t> all(S.size()), used;
  for (size_t r = 0; r < S.size(); ++r) all[r] = (uint32_t)r;
  std::vector<double> m;
  median_of(aligned, all, K, &m);
  double gate = gate_px;
  if (!(gate > 0)) {   // half the least distance between lattice neighbours of m0
    double least = -1;
    for (uint32_t i = 0; i < R; ++i)
      for (uint32_t j = 0; j < C; ++j)
        for (int dir = 0; dir < 2; ++dir) {
          const uint32_t i2 = i + (dir == 0), j2 = j + (dir == 1);
          if (i2 >= R || j2 >= C) continue;
          const double du = m[2 * (i2 * C + j2)] - m[2 * (i * C + j)], dv = m[2 * (i2 * C + j2) + 1] - m[2 * (i * C + j) + 1];
          const double d = std::sqrt(du * du + dv * dv);
          if (least < 0 || d < least) least = d;
        }
    gate = least / 2;
  }
  out->gate = gate;
  const double gate2 = gate * gate;
  std::vector<double> d2(S.size());
  for (size_t r = 0; r < S.size(); ++r) {
    d2[r] = max_d2(aligned, (uint32_t)r, m.data(), N, nullptr);
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

  // 6. the median of the used images and the spread around it
  median_of(aligned, used, K, &m);
  for (uint32_t k = 0; k < K; ++k) out->xy[k] = m[k];
  double worst = 0, sum = 0;
  for (uint32_t r : used) {
    const double w = max_d2(aligned, r, m.data(), N, &sum);
    if (w > worst) worst = w;
  }
  out->spread_max = std::sqrt(worst);
  out->spread_rms = std::sqrt(sum / ((double)used.size() * (double)N));
  if (dist_out)
    for (size_t r = 0; r < S.size(); ++r) dist_out[S[r]] = std::sqrt(max_d2(aligned, (uint32_t)r, m.data(), N, nullptr));
  return ILCC_OK;
}

}  // namespace

extern "C" int32_t ilcc_fuse_image_corners(const double* xy, const int32_t* rows, const int32_t* cols, const uint8_t* accepted, uint32_t n,
                                           uint32_t a, uint32_t b, double gate_px, ilcc_fused_image_corners* out, uint8_t* used_out,
                                           double* dist_out) {
  if (!out) return ILCC_BAD_ARGUMENT;
  std::memset(out, 0, sizeof(*out));
  out->ref_image = -1;
  out->n_images = (int32_t)n;
  int32_t st;
  if ((n && (!xy || !rows || !cols || !accepted)) || a < 3 || b < 3 || (uint64_t)a * b > ILCC_MAX_CORNERS || !std::isfinite(gate_px)) {
    st = ILCC_BAD_ARGUMENT;
  } else {
    try {   // no exception crosses the C-ABI
      st = fuse(xy, rows, cols, accepted, n, a, b, gate_px, out, used_out, dist_out);
    } catch (...) {
      st = ILCC_IO_ERROR;
    }
  }
  out->status = st;
  return st;
}

extern "C" int32_t ilcc_image_sequence_cut(const uint64_t* raw_bytes, uint32_t n, uint64_t device_bytes_per_image, uint64_t staging_bytes,
                                           uint64_t device_bytes, uint32_t* batch_first, uint32_t* n_batches) {
  if ((n && !raw_bytes) || !batch_first || !n_batches) return ILCC_BAD_ARGUMENT;
  const uint64_t staging = staging_bytes ? staging_bytes : kDefaultStagingBytes, device = device_bytes ? device_bytes : kDefaultDeviceBytes;
  *n_batches = 0;
  batch_first[0] = 0;
  uint64_t raw = 0, dev = 0;
  uint32_t in_batch = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t r = (raw_bytes[i] + 255u) & ~(uint64_t)255u;   // a frame starts on a 256-byte boundary of the blob
    if (r > staging || device_bytes_per_image > device) return ILCC_CAPACITY;
    if (in_batch && (raw + r > staging || dev + device_bytes_per_image > device)) {
      batch_first[++*n_batches] = i;
      raw = dev = 0;
      in_batch = 0;
    }
    raw += r;
    dev += device_bytes_per_image;
    ++in_batch;
  }
  if (in_batch) batch_first[++*n_batches] = n;
  return ILCC_OK;
}
