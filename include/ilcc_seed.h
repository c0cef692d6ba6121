/*
 * ilcc_seed.h -- finding the chessboard in a LiDAR scan without a click (K15, in libilcc_hip.so).
 *
 * Every entry of ilcc_hip.h takes the seed (`click`) from outside: a person in rviz, or an image PnP that needs the extrinsic
 * being computed.  The entries here PROPOSE seeds: one pass over the whole cloud names the few places where a board-sized planar
 * patch stands, and ilcc_extract_auto[_batch] runs the ordinary exact pipeline on each proposal and keeps the first it accepts.
 *
 * What K15 computes (csrc/k15_seed_components.hip).  Everything that decides anything is integer arithmetic, so the result does not
 * depend on thread order and tests/seed_ref.py restates it bit for bit.
 *   quantise   a point with a non-finite x, y or z is dropped.  Otherwise, per axis, t = floorf(v * 1024.0f + 0.5f) in fp32 (unit
 *              2^-10 m; the multiplication is exact), the point is dropped unless |t| <= range_q on every axis, and q = (int32) t.
 *   cell       cq = ceil(cell * 1024) quanta; cell index = FLOOR division q div cq per axis (not truncation: -1 div 123 = -1);
 *              off = ceil(range_q / cq), N = 2 off + 1 <= ILCC_SEED_GRID_MAX; key = (ix + off) + N ((iy + off) + N (iz + off)).
 *   occupied   the keys of a frame go into an open-addressing hash set of ilcc_seed_table_size(points of the frame) slots, home
 *              slot ilcc_seed_hash(key, size), linear probing (+1, wrapping).
 *   components 26-connected components of the occupied cells (union-find over cells; the root of a component is its smallest key).
 *   moments    per component n, sum q (3), sum q q^T (6: xx xy xz yy yz zz) as int64.  |q| <= range_q and a frame of n points give
 *              |sum| <= n range_q^2: 2^17 points at the default 20 m (20 480 quanta) stay below 2^46.  range_q is capped at
 *              floor(sqrt(2^62 / max_total_points)) of the handle, so no sum can leave int64 (the default binds only above 2^33 points).
 *   records    components of n >= cluster_min, at most max_components per frame, as ILCC_SEED_RECORD_WORDS int64 each:
 *              key, n, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz -- sorted by key on the host.
 *
 * Cells of edge >= the clustering tolerance with 26-connectivity contain every Euclidean single-linkage cluster of that tolerance
 * (two points <= tol apart lie in the same or in adjacent cells), so a component is a SUPERSET of the cluster the exact pipeline
 * extracts around a seed inside it.
 *
 * Host finishing (csrc/seed_host.cpp).  Per record: C = (n sum q q^T - sum q sum q^T) exactly in __int128, as double / (n^2 2^20) = the
 * covariance in m^2; centroid = sum q / (1024 n); eigenvalues l0 <= l1 <= l2.  Gates: sqrt(l0) <= max_rms; L1 = sqrt(12 l1) within
 * [size_lo, size_hi] x board_w x grid_length; L2 = sqrt(12 l2) within [size_lo, size_hi] x board_h x grid_length (sqrt(12 var) is
 * the side of a uniformly covered rectangle).  Score = |L1 - W g| / (W g) + |L2 - H g| / (H g); seeds ascend by score, ties by key;
 * at most max_seeds are kept.
 *
 * LIMITS.  A board whose component touches something else -- a hand, a stand, ground closer than two cells -- fails the size gate
 * and is not proposed.  The proposal is the centroid of a superset component, not of the reference's cluster: the pipeline behind
 * it does the exact work, the seed only has to fall within the ROI's reach of the board.
 */
#ifndef ILCC_SEED_H_
#define ILCC_SEED_H_

#include "ilcc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ILCC_SEED_RECORD_WORDS 11   /* int64 per component record */
#define ILCC_SEED_GRID_MAX 1024     /* cells per axis */
#define ILCC_SEED_TABLE_MIN 64      /* smallest hash set */
#define ILCC_SEED_FRAME_POINTS_MAX (1u << 28)

typedef struct ilcc_seed_params {
  double cell;             /* m; default params.cluster_tol (0.12 -> 123 quanta) */
  double range;            /* m; default 20: points beyond it on any axis are dropped */
  int32_t cluster_min;     /* default params.cluster_min: smaller components are not recorded */
  int32_t max_components;  /* records per frame (default 64) */
  int32_t max_seeds;       /* seeds kept per frame (default 4) */
  int32_t board_w, board_h; /* squares, from params */
  int32_t reserved0;
  double grid_length;      /* from params */
  double max_rms;          /* gate on sqrt(l0), m; default params.ransac_thresh */
  double size_lo, size_hi; /* gates on L1, L2 relative to the board's sides (defaults 0.7, 1.3: see DESIGN.md section 9) */
  double max_oob_share;    /* ilcc_extract_auto*: accept only n_oob <= max_oob_share (n_black + n_white) (default 0.05) */
} ilcc_seed_params;

typedef struct ilcc_seed {
  float centroid[3];       /* the seed: use as `click` */
  int32_t n;               /* points of the component */
  double l1, l2;           /* sqrt(12 l1), sqrt(12 l2), m */
  double rms;              /* sqrt(l0), m */
  double score;
  uint32_t key;            /* root key of the component */
  uint32_t reserved0;
} ilcc_seed;

/* slots of a frame's hash set: the smallest power of two >= max(ILCC_SEED_TABLE_MIN, 2 n_points) */
static inline uint32_t ilcc_seed_table_size(uint32_t n_points) {
  uint64_t t = ILCC_SEED_TABLE_MIN;
  while (t < 2ull * n_points) t <<= 1;
  return (uint32_t)t;
}
/* home slot of a key in a set of table_size slots (a power of two >= 2): multiplicative hashing, the top log2(table_size) bits */
static inline uint32_t ilcc_seed_hash(uint32_t key, uint32_t table_size) {
  uint32_t bits = 0;
  while ((1u << bits) < table_size) ++bits;
  return (uint32_t)(key * 2654435761u) >> (32u - bits);
}

void ilcc_default_seed_params(const ilcc_params* p, ilcc_seed_params* sp);

/* bytes of device scratch (256-byte aligned) that serve any batch of at most n_frames frames and total_points points */
uint64_t ilcc_seed_scratch_bytes(uint32_t n_frames, uint64_t total_points, const ilcc_seed_params* sp);

/* Seeds of every frame of a batch resident in HBM (d_xyzi device, offsets host: the layout of ilcc_extract_batch_device).
 * out_seeds: n_frames x sp->max_seeds (host), out_counts: n_frames (host): seeds of the frame, or -ILCC_CAPACITY for a frame with
 * more than max_components components of cluster_min points (its seeds are not written; the other frames are unaffected).
 * d_scratch needs no initialisation and may be reused dirty.  hip_stream: a hipStream_t, NULL = the null stream.  Synchronous on
 * return.  Refusals (ILCC_BAD_ARGUMENT / ILCC_CAPACITY; nothing launched, outputs untouched): null pointers, bad offsets, more
 * frames or points than the handle holds, a frame above ILCC_SEED_FRAME_POINTS_MAX points, range / cell above
 * ILCC_SEED_GRID_MAX cells per axis, non-positive cell / range / counts, scratch not 256-byte aligned. */
int32_t ilcc_propose_seeds_device(ilcc_handle* h, const float* d_xyzi, const uint64_t* offsets, uint32_t n_frames,
                                  const ilcc_seed_params* sp, void* d_scratch, ilcc_seed* out_seeds, int32_t* out_counts,
                                  void* hip_stream);
/* the same with host buffers (allocates the device copy and the scratch for the call) */
int32_t ilcc_propose_seeds(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames,
                           const ilcc_seed_params* sp, ilcc_seed* out_seeds, int32_t* out_counts);

/* Test entry: the sorted integer records of frame `frame` of a batch of host clouds.  out_records: cap_records x
 * ILCC_SEED_RECORD_WORDS int64, *out_n = records written.  d_scratch: NULL (allocated for the call) or the caller's, as above.
 * Returns ILCC_CAPACITY (nothing written) when that frame has more than max_components (or cap_records) records. */
int32_t ilcc_debug_seed_components(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames,
                                   const ilcc_seed_params* sp, void* d_scratch, uint32_t frame, int64_t* out_records,
                                   uint32_t cap_records, int32_t* out_n);

/* Diagnostic: the spans, in ms, of K15's launches -- clear, insert, moments, union, reduce, pack -- in the calling thread's last
 * seed call (HIP events on the call's stream between the launches: no copy, no host work). */
#define ILCC_SEED_LAUNCHES 6
void ilcc_debug_seed_launch_ms(float out[ILCC_SEED_LAUNCHES]);

/* Seeds, then the ordinary pipeline on every candidate.  Cloud f with k_f seeds becomes k_f frames of ONE ordinary batch (device
 * copies of the cloud, one per seed, through ilcc_extract_batch_device -- the existing path runs unchanged), so the handle must hold
 * sum k_f <= max_frames frames and sum k_f n_f <= max_total_points points: create it with max_seeds times the frames and points of
 * the largest call (ILCC_CAPACITY otherwise, nothing written).  Per cloud the first candidate in rank order is taken that has
 * status == ILCC_OK, ILCC_FLAG_LOW_COVERAGE clear and n_oob <= max_oob_share (n_black + n_white): out[f] = its record -- byte for
 * byte what ilcc_extract returns for that cloud with click = out_seed[f] (but grid_ties, which depends on timing in any call; like ilcc_wait, corners beyond the board's count are left
 * as the caller passed them) -- out_seed[3 f ..] = its seed, out_rank[f] = its rank.  A cloud without an accepted candidate gets
 * the best-ranked candidate's record and seed with status ILCC_BOARD_NOT_FOUND and out_rank[f] = -1; a cloud without any candidate
 * (or with more than max_components components) a zero record with that status, n_points set, and a zero seed. */
int32_t ilcc_extract_auto_batch(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames,
                                const ilcc_seed_params* sp, ilcc_result* out, float* out_seed, int32_t* out_rank);
int32_t ilcc_extract_auto(ilcc_handle* h, const float* xyzi, uint32_t n, const ilcc_seed_params* sp, ilcc_result* out,
                          float out_seed[3], int32_t* out_rank);

#ifdef __cplusplus
}
#endif
#endif
