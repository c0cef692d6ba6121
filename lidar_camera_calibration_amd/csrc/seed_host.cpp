// seed_host.cpp -- K15's host half: the integer lattice of a parameter set, and what turns a frame's packed component records into
// ranked seeds (include/ilcc_seed.h).  Plain C++ without HIP: it also builds alone, under sanitizers, for tests/test_seed_cpu.py.
#include <algorithm>
#include <cmath>
#include <vector>

#include "eig3.h"
#include "k15_seed.h"

namespace ilcc {

bool seed_grid(const ilcc_seed_params& sp, uint64_t max_total_points, SeedGrid* g) {
  if (!(sp.cell > 0) || !(sp.range > 0) || !(sp.cell * 1024.0 < 1e9) || !(sp.range * 1024.0 <= 8388608.0)) return false;   // range_q <= 2^23: exact as fp32
  int64_t range_q = (int64_t)std::floor(sp.range * 1024.0);
  // sums of q^2 over max_total_points points stay below 2^62
  const int64_t cap = (int64_t)std::floor(std::sqrt(4611686018427387904.0 / (double)(max_total_points ? max_total_points : 1)));
  range_q = std::min(range_q, cap);
  const int64_t cq = (int64_t)std::ceil(sp.cell * 1024.0);
  if (range_q < 1 || cq < 1) return false;
  const int64_t off = (range_q + cq - 1) / cq;
  if (2 * off + 1 > ILCC_SEED_GRID_MAX) return false;
  g->range_q = (int32_t)range_q;
  g->cq = (int32_t)cq;
  g->off = (int32_t)off;
  g->N = (int32_t)(2 * off + 1);
  return true;
}

int32_t seed_rank(const int64_t* records, int32_t n_rec, const ilcc_seed_params& sp, ilcc_seed* out) {
  const double side1 = sp.board_w * sp.grid_length, side2 = sp.board_h * sp.grid_length;
  std::vector<ilcc_seed> cand;
  for (int32_t r = 0; r < n_rec; ++r) {
    const int64_t* w = records + (int64_t)r * ILCC_SEED_RECORD_WORDS;
    const int64_t n = w[1];
    if (n < 1) continue;
    const __int128 s[3] = {w[2], w[3], w[4]};
    const int64_t ss[3][3] = {{w[5], w[6], w[7]}, {w[6], w[8], w[9]}, {w[7], w[9], w[10]}};
    const double scale = (double)n * (double)n * 1048576.0;
    double cov[9], ev[3], vec[3][3];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) cov[3 * a + b] = (double)((__int128)n * ss[a][b] - s[a] * s[b]) / scale;   // exact up to the one conversion
    eig3_sym(cov, ev, vec);
    ilcc_seed sd{};
    for (int a = 0; a < 3; ++a) sd.centroid[a] = (float)((double)w[2 + a] / ((double)n * 1024.0));
    sd.n = (int32_t)n;
    sd.rms = std::sqrt(std::max(ev[0], 0.0));
    sd.l1 = std::sqrt(12.0 * std::max(ev[1], 0.0));
    sd.l2 = std::sqrt(12.0 * std::max(ev[2], 0.0));
    sd.score = std::fabs(sd.l1 - side1) / side1 + std::fabs(sd.l2 - side2) / side2;
    sd.key = (uint32_t)w[0];
    if (!(sd.rms <= sp.max_rms)) continue;
    if (!(sd.l1 >= sp.size_lo * side1 && sd.l1 <= sp.size_hi * side1)) continue;
    if (!(sd.l2 >= sp.size_lo * side2 && sd.l2 <= sp.size_hi * side2)) continue;
    cand.push_back(sd);
  }
  std::sort(cand.begin(), cand.end(), [](const ilcc_seed& a, const ilcc_seed& b) { return a.score != b.score ? a.score < b.score : a.key < b.key; });
  const int32_t keep = std::min<int32_t>((int32_t)cand.size(), sp.max_seeds);
  for (int32_t k = 0; k < keep; ++k) out[k] = cand[k];
  return keep;
}

bool seed_planar_thresholds(const ilcc_seed_planar_params& pp, double* flat_q2, double* spread_q2, double* own_q2) {
  const double t[3] = {pp.planar_rms, pp.min_spread, pp.own_rms};
  double* out[3] = {flat_q2, spread_q2, own_q2};
  for (int k = 0; k < 3; ++k) {
    if (!(t[k] > 0) || !(t[k] < 1e9)) return false;   // NaN fails too
    const double q = 1024.0 * t[k];
    *out[k] = q * q;
  }
  return true;
}

bool seed_planar_frame_fits(uint64_t n_points, const SeedGrid& g) { return n_points * 2ull * (uint64_t)g.cq < (1ull << 31); }

}  // namespace ilcc

extern "C" void ilcc_default_seed_planar_params(const ilcc_params* p, ilcc_seed_params* sp, ilcc_seed_planar_params* pp) {
  if (!p || !sp || !pp) return;
  ilcc_default_seed_params(p, sp);
  sp->max_rms = 0.05;   // a component of core cells keeps a rim of cells that also hold floor: DESIGN.md section 9
  *pp = ilcc_seed_planar_params{};
  pp->planar_rms = p->ransac_thresh;
  pp->min_spread = sp->cell / 2;
  pp->own_rms = 0.02;
}

extern "C" void ilcc_default_seed_params(const ilcc_params* p, ilcc_seed_params* sp) {
  if (!p || !sp) return;
  *sp = ilcc_seed_params{};
  sp->cell = p->cluster_tol;
  sp->range = 20.0;
  sp->cluster_min = p->cluster_min;
  sp->max_components = 64;
  sp->max_seeds = 4;
  sp->board_w = p->board_w;
  sp->board_h = p->board_h;
  sp->grid_length = p->grid_length;
  sp->max_rms = p->ransac_thresh;
  sp->size_lo = 0.7;
  sp->size_hi = 1.3;
  sp->max_oob_share = 0.05;
}
