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
 * Planar seeds (K15p; the ilcc_*_planar entries).  A second way of forming the components, for a board that touches the ground,
 * a stand or a hand.  Quantisation, cells, the hash set and the per-cell moments are the ones above; then every occupied cell is
 * classified, and the components are the 26-connected components of the CORE cells alone:
 *   block      n_b, sum q, sum q q^T over the occupied cells of the cell's 3 x 3 x 3 block (a neighbour index outside [0, N) on an
 *              axis is skipped, never wrapped), translated exactly, in integers, to the cell's origin o = cq (cell index): q' = q - o,
 *              |q'| <= 2 cq.  C = n_b sum q' q'^T - sum q' sum q'^T is formed in int64: a frame is admitted only while
 *              n_points 2 cq < 2^31 (8.7 M points at the default cell; ILCC_BAD_ARGUMENT beyond).  The six entries of C are converted
 *              to fp64 once each (round to nearest) and eig3_sym (cyclic Jacobi, csrc/eig3.h) gives w0 <= w1 <= w2 and the unit
 *              normal v0.  Everything in fp64 is unfused IEEE + - x / sqrt in the order written here.
 *   flat       w0 <= (n_b n_b) ((1024 planar_rms) (1024 planar_rms))
 *   surface    12 w1 >= (n_b n_b) ((1024 min_spread) (1024 min_spread))      (a single LiDAR ring is a line and has no normal)
 *   own        with m_a = (double) (sum_b q'_a) / n_b, n_o, s_a, ss_ab the cell's OWN translated moments as fp64 (exact), and
 *              A_ab = ((ss_ab - m_a s_b) - m_b s_a) + (n_o m_a) m_b,   r_a = (A_a0 v0_0 + A_a1 v0_1) + A_a2 v0_2:
 *              (v0_0 r_0 + v0_1 r_1) + v0_2 r_2 <= n_o ((1024 own_rms) (1024 own_rms))      (the cell's own points lie in the patch)
 *   core       flat and surface and own.
 *   records    as above, of the core components of n >= cluster_min: the smallest key among the component's core cells, then the
 *              sums over the own points of its core cells.  Gates, score and order are the ordinary ones, with max_rms 0.05 by
 *              default: a component's rim cells still hold some floor.
 * tests/seed_planar_ref.py restates this bit for bit.
 *
 * LIMITS.  The ordinary entries propose a board only when its component touches nothing else: a hand, a stand or ground closer than
 * two cells joins it and fails the size gate.  The planar entries cut the board from a floor it stands on or in, from a pole and
 * from whatever meets it at an angle, because the cells along the joint hold two surfaces and are not core.  Not covered by either:
 * a board parallel to a wall less than two cells away (the block holds both planes); a board so far away that a block holds a single
 * ring (the surface test fails); and anything that is itself a board-sized flat rectangle, which is proposed like a board -- the
 * pipeline behind the seed decides.  The proposal is the centroid of a superset component (ordinary) or of the board's core cells
 * (planar), not of the reference's cluster: the pipeline behind it does the exact work, the seed only has to fall within the ROI's
 * reach of the board.
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

/* ---- planar seeds (K15p): the contract of each entry is its sibling's above; what differs is stated here */

typedef struct ilcc_seed_planar_params {
  double planar_rms;       /* m; a block is flat when its smallest rms extent is at most this (default params.ransac_thresh) */
  double min_spread;       /* m; ... and a surface when sqrt(12 w1) / n_b, the side of its second extent, is at least this (default cell / 2) */
  double own_rms;          /* m; rms distance of the cell's own points from the block's plane through its centroid (default 0.02) */
} ilcc_seed_planar_params;

/* sp as ilcc_default_seed_params sets it, but max_rms = 0.05; pp the defaults above */
void ilcc_default_seed_planar_params(const ilcc_params* p, ilcc_seed_params* sp, ilcc_seed_planar_params* pp);

/* the ordinary scratch followed by one byte per point */
uint64_t ilcc_seed_planar_scratch_bytes(uint32_t n_frames, uint64_t total_points, const ilcc_seed_params* sp);

/* Further refusals (ILCC_BAD_ARGUMENT, nothing launched, outputs untouched): pp null, a threshold that is not positive, a frame of
 * n points with n 2 ceil(1024 cell) >= 2^31.  One scratch buffer of ilcc_seed_planar_scratch_bytes serves planar and ordinary calls
 * in any order. */
int32_t ilcc_propose_seeds_planar_device(ilcc_handle* h, const float* d_xyzi, const uint64_t* offsets, uint32_t n_frames,
                                         const ilcc_seed_params* sp, const ilcc_seed_planar_params* pp, void* d_scratch,
                                         ilcc_seed* out_seeds, int32_t* out_counts, void* hip_stream);
int32_t ilcc_propose_seeds_planar(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames,
                                  const ilcc_seed_params* sp, const ilcc_seed_planar_params* pp, ilcc_seed* out_seeds, int32_t* out_counts);
int32_t ilcc_debug_seed_planar_components(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames,
                                          const ilcc_seed_params* sp, const ilcc_seed_planar_params* pp, void* d_scratch, uint32_t frame,
                                          int64_t* out_records, uint32_t cap_records, int32_t* out_n);

/* the spans of clear, insert, moments, classify, union, reduce, pack in the calling thread's last planar seed call */
#define ILCC_SEED_PLANAR_LAUNCHES 7
void ilcc_debug_seed_planar_launch_ms(float out[ILCC_SEED_PLANAR_LAUNCHES]);

int32_t ilcc_extract_auto_planar_batch(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames,
                                       const ilcc_seed_params* sp, const ilcc_seed_planar_params* pp, ilcc_result* out, float* out_seed,
                                       int32_t* out_rank);
int32_t ilcc_extract_auto_planar(ilcc_handle* h, const float* xyzi, uint32_t n, const ilcc_seed_params* sp,
                                 const ilcc_seed_planar_params* pp, ilcc_result* out, float out_seed[3], int32_t* out_rank);

#ifdef __cplusplus
}
#endif
#endif
