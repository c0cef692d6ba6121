// k15_seed.h -- what K15's kernels (k15_seed_components.hip), its host chain (seed_api.cpp) and the host finishing (seed_host.cpp)
// share.  Plain C++: seed_host.cpp also builds alone, under sanitizers, for tests/test_seed_cpu.py.
#pragma once

#include <stdint.h>

#include <string>

#include "ilcc_seed.h"

namespace ilcc {

constexpr uint32_t kSeedEmpty = 0xFFFFFFFFu;   // an empty slot of the hash set (keys are < 2^30: N <= 1024 per axis)
constexpr int kSeedMoments = 10;               // n, sum q (3), sum q q^T (6) per cell
constexpr int kSeedThreads = 256;

struct SeedFrame {       // one per frame, in the scratch's head
  uint64_t pt_beg;       // first point of the frame in xyzi = first cell slot of the frame in the per-cell arrays (cells <= points)
  uint64_t tab_beg;      // first slot of the frame's hash set
  uint32_t n;            // points
  uint32_t tab_mask;     // slots - 1
  uint32_t tab_shift;    // 32 - log2(slots): home slot = (key * 2654435761u) >> tab_shift
  uint32_t pad;
};

struct SeedGrid {        // the integer lattice of a call
  int32_t range_q, cq, off, N;
};

#ifdef __HIPCC__
struct SeedCtx {         // passed by value to every K15 kernel
  const float4* xyzi;
  const SeedFrame* fr;
  uint32_t n_frames;
  uint32_t cluster_min, max_components;
  SeedGrid g;
  uint64_t slots_total;
  uint32_t* counters;    // per frame: [2 f] occupied cells, [2 f + 1] qualifying components met by the pack
  uint32_t* tab_key;     // hash sets: the cell key, kSeedEmpty = free
  uint32_t* tab_ord;     // ... and the cell's ordinal within its frame (the order of insertion: arbitrary, decides nothing)
  uint32_t* cell_key;    // per cell (frame's pt_beg + ordinal)
  uint32_t* parent;      // union-find over ordinals; key[parent[c]] <= key[c]
  long long* mom;        // kSeedMoments per cell
  long long* packed;     // n_frames x max_components x ILCC_SEED_RECORD_WORDS
  // planar seeds (K15p) only; core == nullptr selects the ordinary components
  uint8_t* core;         // per cell: 1 = CORE (the classify launch writes every occupied cell's flag), behind every ordinary part
  double flat_q2, spread_q2, own_q2;   // (1024 planar_rms)^2, (1024 min_spread)^2, (1024 own_rms)^2: squared thresholds in quanta
};
constexpr int kSeedLaunches = 6;         // clear, insert, moments, union, reduce, pack
constexpr int kSeedPlanarLaunches = 7;   // clear, insert, moments, classify, union, reduce, pack
// between: nullptr, or (launches + 1) events recorded in front of, between and behind the launches: kSeedLaunches of them, or
// kSeedPlanarLaunches where c.core is set
void launch_seed_components(const SeedCtx& c, uint32_t max_frame_points, hipStream_t s, const hipEvent_t* between);   // k15_seed_components.hip
#endif

// ---- ilcc_api.cpp: what the seed entries need of a handle
struct HandleView {
  int device;
  ilcc_params p;
  uint32_t max_frames;
  uint64_t max_points;
};
HandleView handle_view(const ilcc_handle* h);
int32_t handle_fail(ilcc_handle* h, int32_t code, const std::string& what);   // sets ilcc_last_error(h), returns code

// ---- seed_host.cpp
// the lattice of a parameter set; false: non-positive cell / range, or more than ILCC_SEED_GRID_MAX cells per axis
bool seed_grid(const ilcc_seed_params& sp, uint64_t max_total_points, SeedGrid* g);
// gates, score and order on n_rec records (sorted by key): writes at most sp.max_seeds seeds, returns their number
int32_t seed_rank(const int64_t* records, int32_t n_rec, const ilcc_seed_params& sp, ilcc_seed* out);
// K15p: the squared thresholds in quanta, each (1024 t)^2 as two fp64 products; false: a threshold that is not positive and finite
bool seed_planar_thresholds(const ilcc_seed_planar_params& pp, double* flat_q2, double* spread_q2, double* own_q2);
// K15p: whether a frame of n points keeps the block covariance in int64 (n 2 cq < 2^31)
bool seed_planar_frame_fits(uint64_t n_points, const SeedGrid& g);

}  // namespace ilcc
