// K2 seeded_cluster -- replaces pcl::EuclideanClusterExtraction + nearestKSearch of
// LidarCornersEst::EuclideanCluster (/root/reference/ilcc2/src/LidarCornersEst.cpp:124-153).
//
// Single-linkage components of the radius graph (squared float distance dx*dx+dy*dy+dz*dz < (float)(tol*tol),
// FLANN's strict test).  Round 4: the components are built on CELLS, not on points.
//
//   The frame's ROI points are binned into a grid of cells of side s = 0.57 tol.  3 s^2 = 0.975 tol^2, so any two points
//   of one cell pass the distance test (with 2.5 % to spare, against ~1e-5 of float rounding in the binning): a cell is a
//   clique and needs no test at all.  Two points within tol sit at most 2 cells apart on every axis (tol / s = 1.754 < 2),
//   so the components of the points are the components of the graph whose nodes are the occupied cells and whose edges
//   join two cells (within +-2 per axis) that hold at least one pair of points within tol.  A VLP-16 ROI of ~1350 points
//   has ~300 occupied cells and the union-find runs on those: the point-level search of rounds 1-3 tested every point
//   against every candidate of 14 cells of side tol (~250 k distance tests and ~1 k dependent LDS union chains per frame,
//   a 1024-thread / 100 KB workgroup that could not get a CU beside K6); this one probes a bitmap for the occupied
//   neighbours (5 neighbours per 64-bit window read), skips pairs whose cells already share a root and stops a pair's
//   tests at the first hit.  One workgroup of 256 threads (1024 in batches of <= 64 frames), ~50 KB of LDS: bitmap of the
//   padded bounding grid + its rank directory (cell key -> dense cell id), five words per cell, the points sorted by cell
//   (frames above the LDS point capacity keep the sorted points in HBM/L2 -- BASELINE config 5's ~12 k ROI points; and so does
//   every frame of a launch whose batch would not be resident at once with the copy: launch_cluster).
//   Labels are the smallest member index of a component (atomicMin over its cells), sizes are sums of cell counts: the
//   partition, the 1-NN of the click, the reference's choice rule and the index-ordered output are what they were.
//
//   Frames the LDS grid cannot hold (bounding grid above kFineBits cells: the un-cropped clouds of the online caller
//   get_chessboard_by_point, LidarCornersEst.cpp:72-115; or more occupied cells than the handle's capacity) run the same
//   cell-level algorithm with the cells in a hash table in global memory, in the phases hash_setup ... hash_tail: one workgroup
//   per frame (hashed_cluster_frame, round 5), or the k2h_* chain of kernels over the whole chip for the online caller's second
//   tier.  Only frames beyond THAT path's limits (> 65 536 ROI points) take the point-level spatial hash of rounds 1-3, one
//   workgroup (point_level_cluster_frame).
// Cluster choice follows the reference: components with
// cluster_min <= size <= cluster_max, sorted by size (largest = index 0); the one containing
// the exact 1-NN of the click wins, otherwise index 0.  Members are emitted in index order.  Every path ends in the same
// choice and compaction (choose_cluster, compact_cluster).
#include "ilcc_internal.h"

namespace ilcc {

// find with path halving.  Parents only ever point to smaller indices (the larger root is hooked
// under the smaller), so replacing parent[x] by its grandparent keeps it an ancestor: safe against
// concurrent hooks, which only touch roots.
template <typename P>
__device__ __forceinline__ uint32_t uf_find(P* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    const uint32_t gp = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (gp != p) __hip_atomic_store(&parent[x], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
  }
}

template <typename P>
__device__ __forceinline__ void uf_unite(P* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    // hook the larger root under the smaller one
    const uint32_t old = atomicCAS(&parent[a], a, b);
    if (old == a) return;
  }
}

// bucket of an integer cell; different cells may share a bucket (a far cell's points then simply
// fail the distance test)
__device__ __forceinline__ uint32_t cell_hash(int cx, int cy, int cz) {
  const uint32_t h = (uint32_t)cx * 73856093u ^ (uint32_t)cy * 19349663u ^ (uint32_t)cz * 83492791u;
  return h & (uint32_t)(kClusterHashSize - 1);
}

struct NnKey {
  float d2;
  uint32_t idx;
};
__device__ __forceinline__ bool nn_less(const NnKey& x, const NnKey& y) {
  return x.d2 < y.d2 || (x.d2 == y.d2 && x.idx < y.idx);
}

// ------------------------------------------------------------------ shared by every path
// bounding box of P[0, M) over the workgroup, returned to every thread.  scratch: 112 floats (reusable on return)
__device__ __forceinline__ void block_bbox(const float4* __restrict__ P, uint32_t M, float* scf, float3& lo, float3& hi) {
  const uint32_t tid = threadIdx.x, kT = blockDim.x;
  lo = make_float3(3.0e38f, 3.0e38f, 3.0e38f);
  hi = make_float3(-3.0e38f, -3.0e38f, -3.0e38f);
  for (uint32_t i = tid; i < M; i += kT) {
    const float4 q = P[i];
    lo.x = fminf(lo.x, q.x); lo.y = fminf(lo.y, q.y); lo.z = fminf(lo.z, q.z);
    hi.x = fmaxf(hi.x, q.x); hi.y = fmaxf(hi.y, q.y); hi.z = fmaxf(hi.z, q.z);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo.x = fminf(lo.x, __shfl_xor(lo.x, o, ILCC_WAVE)); lo.y = fminf(lo.y, __shfl_xor(lo.y, o, ILCC_WAVE));
    lo.z = fminf(lo.z, __shfl_xor(lo.z, o, ILCC_WAVE));
    hi.x = fmaxf(hi.x, __shfl_xor(hi.x, o, ILCC_WAVE)); hi.y = fmaxf(hi.y, __shfl_xor(hi.y, o, ILCC_WAVE));
    hi.z = fmaxf(hi.z, __shfl_xor(hi.z, o, ILCC_WAVE));
  }
  __syncthreads();
  if (lane_id() == 0) {
    scf[wave_id()] = lo.x; scf[16 + wave_id()] = lo.y; scf[32 + wave_id()] = lo.z;
    scf[64 + wave_id()] = hi.x; scf[80 + wave_id()] = hi.y; scf[96 + wave_id()] = hi.z;
  }
  __syncthreads();
  for (int w = 0; w < (int)(kT / ILCC_WAVE); ++w) {
    lo.x = fminf(lo.x, scf[w]); lo.y = fminf(lo.y, scf[16 + w]); lo.z = fminf(lo.z, scf[32 + w]);
    hi.x = fmaxf(hi.x, scf[64 + w]); hi.y = fmaxf(hi.y, scf[80 + w]); hi.z = fmaxf(hi.z, scf[96 + w]);
  }
  __syncthreads();
}

// The tail of every path, on the components k < n_comp of a frame's points P[0, M): comp(k, size, min_index) is true when k is
// a component (a root) and then gives its size and smallest member index; label(i, q) is the component of point i (q = P[i]).
// choose_cluster: the exact 1-NN of the click (float squared distance, ties -> lowest index); the largest admissible component
// (ties -> smallest member index), i.e. sorted index 0; the one holding the 1-NN wins when it is admissible.  Writes
// found_board.  Scratch: sc[0, 80) and sc[120, 124).
struct ClusterChoice {
  uint32_t chosen;   // the component to emit
  bool any;          // some component is admissible (else the frame has no cluster)
  bool found;        // the click's 1-NN lies in an admissible component
  float nn_d2;       // squared distance from the click to its 1-NN
};
template <typename Comp, typename Label>
__device__ __forceinline__ ClusterChoice choose_cluster(const Ctx& c, uint32_t f, float3 click, const float4* __restrict__ P,
                                                        uint32_t M, uint32_t n_comp, Comp comp, Label label, uint32_t* sc) {
  const uint32_t tid = threadIdx.x, kT = blockDim.x;
  NnKey best{3.402823466e38f, 0xFFFFFFFFu};
  for (uint32_t i = tid; i < M; i += kT) {
    const float4 q = P[i];
    const float dx = q.x - click.x, dy = q.y - click.y, dz = q.z - click.z;
    float d2 = dx * dx;
    d2 = d2 + dy * dy;
    d2 = d2 + dz * dz;
    const NnKey k{d2, i};
    if (nn_less(k, best)) best = k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    NnKey t;
    t.d2 = __shfl_down(best.d2, o, ILCC_WAVE);
    t.idx = __shfl_down(best.idx, o, ILCC_WAVE);
    if (nn_less(t, best)) best = t;
  }
  const uint32_t cmin_sz = (uint32_t)c.p.cluster_min, cmax_sz = (uint32_t)c.p.cluster_max;
  uint32_t bsz = 0, bidx = 0xFFFFFFFFu, broot = 0xFFFFFFFFu;
  for (uint32_t k = tid; k < n_comp; k += kT) {
    uint32_t sz, mi;
    if (!comp(k, sz, mi)) continue;
    if (sz < cmin_sz || sz > cmax_sz) continue;
    if (sz > bsz || (sz == bsz && mi < bidx)) {
      bsz = sz;
      bidx = mi;
      broot = k;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t s2 = __shfl_down(bsz, o, ILCC_WAVE), i2 = __shfl_down(bidx, o, ILCC_WAVE), r2 = __shfl_down(broot, o, ILCC_WAVE);
    if (s2 > bsz || (s2 == bsz && i2 < bidx)) {
      bsz = s2;
      bidx = i2;
      broot = r2;
    }
  }
  float* scf = reinterpret_cast<float*>(sc);
  __syncthreads();
  if (lane_id() == 0) {
    scf[wave_id()] = best.d2;
    sc[16 + wave_id()] = best.idx;
    sc[32 + wave_id()] = bsz;
    sc[48 + wave_id()] = bidx;
    sc[64 + wave_id()] = broot;
  }
  __syncthreads();
  if (tid == 0) {
    NnKey nb{scf[0], sc[16]};
    uint32_t s0 = sc[32], i0 = sc[48], r0 = sc[64];
    for (int w = 1; w < (int)(kT / ILCC_WAVE); ++w) {
      const NnKey k{scf[w], sc[16 + w]};
      if (nn_less(k, nb)) nb = k;
      const uint32_t s2 = sc[32 + w], i2 = sc[48 + w], r2 = sc[64 + w];
      if (s2 > s0 || (s2 == s0 && i2 < i0)) {
        s0 = s2;
        i0 = i2;
        r0 = r2;
      }
    }
    // a click with a NaN or infinite component is at no comparable distance from any point: no candidate ever beat the initial
    // key.  The reference's search then keeps its initial index, point 0 (and P[0xFFFFFFFF] is far outside the frame)
    if (nb.idx == 0xFFFFFFFFu) nb.idx = 0u;
    const uint32_t nn_root = label(nb.idx, P[nb.idx]);
    uint32_t nsz = 0, nmi;
    comp(nn_root, nsz, nmi);
    const bool found = nsz >= cmin_sz && nsz <= cmax_sz;   // find_board of get_chessboard_by_point (:91-102)
    c.res[f].found_board = found ? 1 : 0;
    sc[120] = found ? nn_root : r0;                         // cluster containing the click's NN, else plane_index = 0
    sc[121] = (s0 == 0) ? 0u : 1u;
    sc[122] = found ? 1u : 0u;
    scf[123] = nb.d2;
  }
  __syncthreads();
  return ClusterChoice{sc[120], sc[121] != 0u, sc[122] != 0u, scf[123]};
}

// stable compaction of the chosen component (index order) into dst; kept(q) sees every point emitted.  Returns their number.
// Scratch: sc[128, 144).
template <typename Label, typename Kept>
__device__ __forceinline__ uint32_t compact_cluster(const float4* __restrict__ P, uint32_t M, uint32_t chosen, Label label,
                                                    float4* __restrict__ dst, uint32_t* sc, Kept kept) {
  uint32_t running = 0;
  for (uint32_t base = 0; base < M; base += blockDim.x) {
    const uint32_t i = base + threadIdx.x;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    bool keep = false;
    if (i < M) {
      q = P[i];
      keep = label(i, q) == chosen;
    }
    if (keep) kept(q);
    uint32_t tot;
    const uint32_t rank = block_rank(keep, sc + 128, tot);
    if (keep) dst[running + rank] = q;
    running += tot;
  }
  return running;
}

// choice and compaction for the paths without a caller-specific check: the frame's result (status or n_cluster)
template <typename Comp, typename Label>
__device__ __forceinline__ void cluster_tail(const Ctx& c, uint32_t f, const float4* __restrict__ P, uint32_t M, uint32_t n_comp,
                                             Comp comp, Label label, uint32_t* sc) {
  const float3 click = make_float3(c.clicks[3 * f], c.clicks[3 * f + 1], c.clicks[3 * f + 2]);
  const ClusterChoice ch = choose_cluster(c, f, click, P, M, n_comp, comp, label, sc);
  if (!ch.any) {
    if (threadIdx.x == 0) c.res[f].status = ILCC_NO_CLUSTER;
    return;
  }
  const uint32_t n = compact_cluster(P, M, ch.chosen, label, c.cluster + c.off[f], sc, [](const float4&) {});
  if (threadIdx.x == 0) c.res[f].n_cluster = (int32_t)n;
}

// ------------------------------------------------------------------ point-level spatial hash (frames beyond the limits of the cell paths)
__device__ __forceinline__ void big_cell(const Ctx& c, const float4& q, int& cx, int& cy, int& cz) {
  const float inv_cell = 1.0f / ((float)c.p.cluster_tol * 1.001f);   // cells of slightly more than the tolerance
  cx = (int)floorf(q.x * inv_cell);
  cy = (int)floorf(q.y * inv_cell);
  cz = (int)floorf(q.z * inv_cell);
}

// spatial hash of a frame: buckets chained through `next` (bucket order depends on the race of the insertions, the
// resulting partition does not)
__device__ __forceinline__ void big_insert_point(const Ctx& c, uint32_t f, uint32_t i) {
  const uint64_t beg = c.off[f];
  uint32_t* head = c.uf_hash_head + (uint64_t)f * kClusterHashSize;
  int cx, cy, cz;
  big_cell(c, c.roi[beg + i], cx, cy, cz);
  c.uf_hash_next[beg + i] = atomicExch(&head[cell_hash(cx, cy, cz)], i);
}

// point i tests the 27 cells around its own; pairs within the tolerance whose parents differ are united
__device__ __forceinline__ void big_search_point(const Ctx& c, uint32_t f, uint32_t i, float tol2) {
  const uint64_t beg = c.off[f];
  const float4* __restrict__ P = c.roi + beg;
  uint32_t* parent = c.uf_parent + beg;
  const uint32_t* head = c.uf_hash_head + (uint64_t)f * kClusterHashSize;
  const uint32_t* next = c.uf_hash_next + beg;
  const float4 pi = P[i];
  int cx, cy, cz;
  big_cell(c, pi, cx, cy, cz);
  // the point's own cell (pairs once: j < i) and its 13 forward neighbours (every pair of adjacent cells is met once, from
  // the cell that comes first in (dz, dy, dx) order); two cells sharing a bucket only add distance tests that fail or repeat
  for (int r = 13; r < 27; ++r) {
      {
        const int dz = r / 9 - 1, dy = (r / 3) % 3 - 1, dx = r % 3 - 1;
        uint32_t j = __hip_atomic_load(&head[cell_hash(cx + dx, cy + dy, cz + dz)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (j != 0xFFFFFFFFu) {
          if (r != 13 ? j != i : j < i) {
            const float4 q = P[j];
            const float ex = q.x - pi.x, ey = q.y - pi.y, ez = q.z - pi.z;
            float d2 = ex * ex;
            d2 = d2 + ey * ey;
            d2 = d2 + ez * ez;
            if (d2 < tol2) {
              const uint32_t qi = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              const uint32_t qj = __hip_atomic_load(&parent[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              if (qi != qj) uf_unite(parent, i, j);
            }
          }
          j = next[j];
        }
      }
  }
}

// the point-level spatial hash of rounds 1-3 by ONE workgroup: the last resort for frames beyond the limits of the cell paths.
// Components are the points that are roots (the smallest member index), their sizes counted on the root.
__device__ void point_level_cluster_frame(const Ctx& c, uint32_t f, uint32_t* sc) {
  const uint64_t beg = c.off[f];
  const uint32_t M = (uint32_t)c.res[f].n_roi, tid = threadIdx.x, kT = blockDim.x;
  uint32_t* parent = c.uf_parent + beg;
  uint32_t* count = c.uf_count + beg;
  uint32_t* head = c.uf_hash_head + (uint64_t)f * kClusterHashSize;
  for (uint32_t i = tid; i < M; i += kT) {
    parent[i] = i;
    count[i] = 0u;
  }
  for (uint32_t k = tid; k < (uint32_t)kClusterHashSize; k += kT) head[k] = 0xFFFFFFFFu;
  __threadfence_block();
  __syncthreads();
  for (uint32_t i = tid; i < M; i += kT) big_insert_point(c, f, i);
  __threadfence_block();
  __syncthreads();
  const float tol2 = (float)(c.p.cluster_tol * c.p.cluster_tol);
  for (uint32_t i = tid; i < M; i += kT) big_search_point(c, f, i, tol2);
  __threadfence_block();
  __syncthreads();
  // ---- flatten: label = root (smallest member index)
  for (uint32_t base = 0; base < M; base += kT) {
    const uint32_t i = base + tid;
    uint32_t root = 0;
    if (i < M) root = uf_find(parent, i);
    __syncthreads();
    if (i < M) parent[i] = root;
    __syncthreads();
  }
  // ---- component sizes (wave-aggregated atomics on the root's counter)
  for (uint32_t base = 0; base < M; base += kT) {
    const uint32_t i = base + tid;
    const bool v = i < M;
    const uint32_t lab = v ? parent[i] : 0xFFFFFFFFu;
    unsigned long long todo = __ballot(v);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const uint32_t ll = __shfl(lab, leader, ILCC_WAVE);
      const unsigned long long same = __ballot(v && lab == ll);
      if (lane_id() == leader) atomicAdd(&count[ll], (uint32_t)__popcll(same));
      todo &= ~same;
    }
  }
  __syncthreads();
  cluster_tail(c, f, c.roi + beg, M, M,
               [&](uint32_t k, uint32_t& sz, uint32_t& mi) {
                 if (parent[k] != k) return false;
                 sz = __hip_atomic_load(&count[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                 mi = k;
                 return true;
               },
               [&](uint32_t i, const float4&) { return parent[i]; }, sc);
}

// ------------------------------------------------------------------ components on cells (the ROI case)
constexpr int kFineBitsOnline = 128 * 1024;      // ... in the first tier of the online caller: a +-1.25 m window at tol 0.10 is <= 49^3 = 118 k cells padded
constexpr int kFineBits = 96 * 1024;             // cells of the padded bounding grid the bitmap holds (12 KiB); a 2 x 3 x 4 m ROI box at
                                                 // tol 0.12 is <= 34 x 48 x 63 = 102 k cells padded, the bounding box of real ROI clouds ~50 k
__host__ __device__ inline uint32_t fine_words(uint32_t bits) { return bits / 32u + 2u; }   // + 2: the 5-bit neighbour windows read one word past their own
constexpr float kFineCellOverTol = 0.57f;        // s / tol: 3 s^2 = 0.9747 tol^2 < tol^2 (cell = clique), tol / s = 1.754 < 2 (neighbours within +-2 cells)
// the 13 forward (dy, dz) rows of the 5 x 5 x 5 neighbourhood, nearest first: row 0 is the cell's own row (dx = +1, +2), every
// other row a window of five cells dx = -2..2.  A pair of cells is met once, from the one with the smaller (z, y, x).
__device__ const signed char kRowDy[13] = {0, 1, 0, 1, -1, 2, 0, 2, -2, 1, -1, 2, -2};
__device__ const signed char kRowDz[13] = {0, 0, 1, 1, 1, 0, 2, 1, 1, 2, 2, 2, 2};

struct FineGrid {
  float3 lo;
  float inv;
  int nx, ny, nz;
};
__device__ __forceinline__ uint32_t fine_key(const FineGrid& g, const float4& q) {
  // + 2: two cells of padding on every side, so that key + (dx, dy, dz) never leaves the grid
  const int cx = (int)floorf((q.x - g.lo.x) * g.inv) + 2, cy = (int)floorf((q.y - g.lo.y) * g.inv) + 2,
            cz = (int)floorf((q.z - g.lo.z) * g.inv) + 2;
  return (uint32_t)(cx + g.nx * (cy + g.ny * cz));
}
// dense id of an occupied cell: set bits below its key (rank directory per 64-bit word)
__device__ __forceinline__ uint32_t fine_rank(const uint32_t* bm, const uint16_t* pre, uint32_t key) {
  const unsigned long long w = reinterpret_cast<const unsigned long long*>(bm)[key >> 6];
  return (uint32_t)pre[key >> 6] + (uint32_t)__popcll(w & ((1ull << (key & 63u)) - 1ull));
}

// exclusive scan over the workgroup of one value per thread (thread order); total via ref.  scratch: >= 17 words.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* scratch, uint32_t& total) {
  uint32_t incl = v;
#pragma unroll
  for (int o = 1; o < ILCC_WAVE; o <<= 1) {
    const uint32_t t = __shfl_up(incl, o, ILCC_WAVE);
    if (lane_id() >= o) incl += t;
  }
  const int nw = (int)(blockDim.x / ILCC_WAVE);
  __syncthreads();
  if (lane_id() == ILCC_WAVE - 1) scratch[wave_id()] = incl;
  __syncthreads();
  uint32_t base = 0, tot = 0;
  for (int w = 0; w < nw; ++w) {
    const uint32_t cw = scratch[w];
    if (w < wave_id()) base += cw;
    tot += cw;
  }
  total = tot;
  return base + incl - v;
}

struct FineLds {
  uint32_t* sc;      // 160 words of scratch
  uint32_t* bm;      // fine_words(cluster_bits): occupancy bitmap of the padded bounding grid
  uint16_t* pre;     // cluster_bits / 64: occupied cells below each 64-bit word
  uint32_t *ckey, *cstart, *ccnt, *cmin, *cpar;   // per occupied cell (capacity c.cluster_cells_cap; cstart one more)
  float *sx, *sy, *sz;   // the points sorted by cell (capacity c.cluster_lds_points; 0 in a launch that keeps them in `cluster`)
};

// point `at` of the cell-sorted copy, in either home
template <bool PTS_LDS>
__device__ __forceinline__ float3 sorted_point(const FineLds& L, const float4* gpts, uint32_t at) {
  if (PTS_LDS) return make_float3(L.sx[at], L.sy[at], L.sz[at]);
  const float4 q = gpts[at];
  return make_float3(q.x, q.y, q.z);
}
#ifndef ILCC_K2_PAIR_GROUP
#define ILCC_K2_PAIR_GROUP 4       // (A/B builds: tools/build_variant.sh)
#endif
#ifndef ILCC_K2_PAIR_GROUP_LDS
#define ILCC_K2_PAIR_GROUP_LDS 4
#endif
// points of B an edge test loads at once, the sorted points in `cluster` / in LDS
constexpr uint32_t kPairGroup = ILCC_K2_PAIR_GROUP, kPairGroupLds = ILCC_K2_PAIR_GROUP_LDS;

// Returns false (uniformly) when the frame does not fit the grid / the cell capacity: the caller takes the point-level path.
template <bool PTS_LDS>
__device__ bool fine_cluster_frame(const Ctx& c, uint32_t f, const FineLds& L) {
  ilcc_result* r = &c.res[f];
  const uint32_t M = (uint32_t)r->n_roi;
  const uint64_t beg = c.off[f];
  const float4* __restrict__ P = c.roi + beg;
  float4* gpts = c.cluster + beg;   // PTS_LDS = false: the sorted points live here until the compaction overwrites it
  const uint32_t tid = threadIdx.x, kT = blockDim.x;
  const float tol2 = (float)(c.p.cluster_tol * c.p.cluster_tol);
  uint32_t* sc = L.sc;
  unsigned long long* stats = c.grid_iters + 3 * kIterSlots;   // [0] most occupied cells a frame needed

  // ---- bounding box
  float3 lo, hi;
  block_bbox(P, M, reinterpret_cast<float*>(sc), lo, hi);
  FineGrid g;
  g.lo = lo;
  g.inv = 1.0f / ((float)c.p.cluster_tol * kFineCellOverTol);
  const float ex = (hi.x - lo.x) * g.inv, ey = (hi.y - lo.y) * g.inv, ez = (hi.z - lo.z) * g.inv;
  if (!(ex < 8192.f && ey < 8192.f && ez < 8192.f)) return false;   // (also catches a NaN extent)
  g.nx = (int)floorf(ex) + 5;
  g.ny = (int)floorf(ey) + 5;
  g.nz = (int)floorf(ez) + 5;
  const unsigned long long cells = (unsigned long long)g.nx * (unsigned long long)g.ny * (unsigned long long)g.nz;
  if (cells > (unsigned long long)c.cluster_bits) return false;
  const uint32_t n_w32 = ((uint32_t)cells + 31u) / 32u + 2u, n_w64 = ((uint32_t)cells + 63u) / 64u;

  // ---- occupancy bitmap, rank directory
  for (uint32_t k = tid; k < ((n_w32 + 1u) & ~1u); k += kT) L.bm[k] = 0u;
  __syncthreads();
  for (uint32_t i = tid; i < M; i += kT) {
    const uint32_t key = fine_key(g, P[i]);
    atomicOr(&L.bm[key >> 5], 1u << (key & 31u));
  }
  __syncthreads();
  uint32_t C = 0;
  {
    const unsigned long long* bm64 = reinterpret_cast<const unsigned long long*>(L.bm);
    const uint32_t per = (n_w64 + kT - 1u) / kT, w0 = tid * per, w1 = min(n_w64, w0 + per);
    uint32_t sum = 0;
    for (uint32_t w = w0; w < w1; ++w) sum += (uint32_t)__popcll(bm64[w]);
    uint32_t run = block_excl_scan(sum, sc, C);
    if (C <= c.cluster_cells_cap)
      for (uint32_t w = w0; w < w1; ++w) {
        L.pre[w] = (uint16_t)run;
        run += (uint32_t)__popcll(bm64[w]);
      }
  }
  if (tid == 0) atomicMax(&stats[0], (unsigned long long)C);
  if (C > c.cluster_cells_cap) return false;   // more occupied cells than the handle's LDS arrays hold: it grows them for the next batch
  __syncthreads();

  // ---- points per cell, smallest member index, key of every occupied cell
  for (uint32_t k = tid; k < C; k += kT) {
    L.ccnt[k] = 0u;
    L.cmin[k] = 0xFFFFFFFFu;
  }
  __syncthreads();
  for (uint32_t i = tid; i < M; i += kT) {
    const uint32_t key = fine_key(g, P[i]);
    const uint32_t cid = fine_rank(L.bm, L.pre, key);
    atomicAdd(&L.ccnt[cid], 1u);
    atomicMin(&L.cmin[cid], i);
    L.ckey[cid] = key;   // (every point of the cell writes the same word)
  }
  __syncthreads();
  {   // exclusive scan of the counts: cstart[k] = first sorted position of cell k
    const uint32_t per = (C + kT - 1u) / kT, k0 = tid * per, k1 = min(C, k0 + per);
    uint32_t sum = 0, tot;
    for (uint32_t k = k0; k < k1; ++k) sum += L.ccnt[k];
    uint32_t run = block_excl_scan(sum, sc, tot);
    for (uint32_t k = k0; k < k1; ++k) {
      L.cstart[k] = run;
      run += L.ccnt[k];
    }
    if (tid == 0) L.cstart[C] = M;
  }
  __syncthreads();
  // placement (the order inside a cell is the race of the atomics: nothing below depends on it); leaves ccnt all zero
  for (uint32_t i = tid; i < M; i += kT) {
    const float4 q = P[i];
    const uint32_t cid = fine_rank(L.bm, L.pre, fine_key(g, q));
    const uint32_t at = L.cstart[cid] + (atomicSub(&L.ccnt[cid], 1u) - 1u);
    if (PTS_LDS) {
      L.sx[at] = q.x;
      L.sy[at] = q.y;
      L.sz[at] = q.z;
    } else {
      gpts[at] = q;
    }
  }
  for (uint32_t k = tid; k < C; k += kT) L.cpar[k] = k;
  if (!PTS_LDS) __threadfence_block();
  __syncthreads();

  // ---- edges between cells.  (row, cell) items, rows outermost: by the time the far rows come up most cells of a
  // surface already share a root and a pair costs two finds.
  for (int row = 0; row < 13; ++row) {
    const int delta = (int)kRowDy[row] * g.nx + (int)kRowDz[row] * g.nx * g.ny;
    for (uint32_t A = tid; A < C; A += kT) {
      const uint32_t lo_bit = (uint32_t)((int)L.ckey[A] + delta - 2);
      const uint32_t w = lo_bit >> 5, sh = lo_bit & 31u;
      uint32_t bits = (uint32_t)((((unsigned long long)L.bm[w + 1] << 32) | (unsigned long long)L.bm[w]) >> sh) & 31u;
      if (row == 0) bits &= 24u;   // the cell's own row: only dx = +1, +2
      if (!bits) continue;
      const uint32_t a0 = L.cstart[A], a1 = L.cstart[A + 1];
      while (bits) {
        const uint32_t b = (uint32_t)__ffs((int)bits) - 1u;
        bits &= bits - 1u;
        const uint32_t B = fine_rank(L.bm, L.pre, lo_bit + b);
        const uint32_t ra = uf_find(L.cpar, A), rb = uf_find(L.cpar, B);
        if (ra == rb) continue;   // same component already (for good)
        const uint32_t b0 = L.cstart[B], b1 = L.cstart[B + 1];
        // A's point once per ia, B's points kGroup at a time: the group's loads are unconditional (an index past the cell's
        // end reads its last point again: harmless) and independent, one round trip per group instead of one per test -- at L2
        // latency (the points in `cluster`) the serial walk was the frame's chain.  Same tests, same arithmetic; which pair hits
        // first does not matter, only whether one does
        constexpr uint32_t kGroup = PTS_LDS ? kPairGroupLds : kPairGroup;
        bool hit = false;
        for (uint32_t ia = a0; ia < a1 && !hit; ++ia) {
          const float3 p = sorted_point<PTS_LDS>(L, gpts, ia);
          for (uint32_t ib = b0; ib < b1 && !hit; ib += kGroup) {
            float3 q[kGroup];
#pragma unroll
            for (uint32_t k = 0; k < kGroup; ++k) q[k] = sorted_point<PTS_LDS>(L, gpts, min(ib + k, b1 - 1u));
            float nearest = 3.0e38f;   // of the group: some d2 < tol2 <=> their minimum is (fminf passes over a NaN as the compare does)
#pragma unroll
            for (uint32_t k = 0; k < kGroup; ++k) {
              const float ex2 = q[k].x - p.x, ey2 = q[k].y - p.y, ez2 = q[k].z - p.z;
              float d2 = ex2 * ex2;
              d2 = d2 + ey2 * ey2;
              d2 = d2 + ez2 * ez2;
              nearest = fminf(nearest, d2);
            }
            hit = nearest < tol2;
          }
        }
        if (hit) uf_unite(L.cpar, ra, rb);
      }
    }
  }
  __syncthreads();

  // ---- components: root of every cell, size and smallest member index on the root (ccnt is zero since the placement;
  // ckey is free now and takes the component's smallest index)
  for (uint32_t base = 0; base < C; base += kT) {
    const uint32_t k = base + tid;
    uint32_t root = 0;
    if (k < C) root = uf_find(L.cpar, k);
    __syncthreads();
    if (k < C) {
      L.cpar[k] = root;
      L.ckey[k] = 0xFFFFFFFFu;
    }
    __syncthreads();
  }
  for (uint32_t k = tid; k < C; k += kT) {
    const uint32_t root = L.cpar[k];
    atomicAdd(&L.ccnt[root], L.cstart[k + 1] - L.cstart[k]);
    atomicMin(&L.ckey[root], L.cmin[k]);
  }
  __syncthreads();

  // ---- exact 1-NN of the click, the choice (components: root cells; a point's: its cell's root)
  const auto comp = [&](uint32_t k, uint32_t& sz, uint32_t& mi) {
    if (L.cpar[k] != k) return false;
    sz = L.ccnt[k];
    mi = L.ckey[k];
    return true;
  };
  const auto label = [&](uint32_t, const float4& q) { return L.cpar[fine_rank(L.bm, L.pre, fine_key(g, q))]; };
  const float kx = c.clicks[3 * f], ky = c.clicks[3 * f + 1], kz = c.clicks[3 * f + 2];
  const ClusterChoice ch = choose_cluster(c, f, make_float3(kx, ky, kz), P, M, C, comp, label, sc);
  // First tier of the online caller: the points are a WINDOW of +-w around the click, the answer must be the whole cloud's.
  // It is, when (1) the window's nearest point is the cloud's -- nothing outside the window is nearer than w; (2) that point's
  // component is admissible -- otherwise the reference falls back to the LARGEST component of the cloud, which a window cannot
  // know; (3) the component is complete -- checked below: no member within tol (+ 1 mm) of the window's faces, so no point
  // outside the window is within tol of it.  Anything else: the second tier clusters the whole cloud.
  if (c.online_tier == 1u) {
    const float w = c.online_window - 1e-3f;   // (the window's faces are float-rounded: a point outside is farther than this)
    if (!(ch.found && ch.nn_d2 <= w * w)) {
      if (tid == 0) c.frame_flags[f] = 1u;
      return true;
    }
  }
  if (!ch.any) {
    if (tid == 0) r->status = ILCC_NO_CLUSTER;
    return true;
  }

  // ---- stable compaction of the chosen component (index order)
  const float safe = c.online_window - ((float)c.p.cluster_tol + 1e-3f);   // (first tier of the online caller: completeness)
  bool near_face = false;
  const uint32_t n = compact_cluster(P, M, ch.chosen, label, c.cluster + beg, sc, [&](const float4& q) {
    near_face |= !(fabsf(q.x - kx) <= safe && fabsf(q.y - ky) <= safe && fabsf(q.z - kz) <= safe);
  });
  if (c.online_tier == 1u) {
    uint32_t tot;
    (void)block_rank(near_face, sc + 128, tot);
    if (tot != 0u) {   // the component may continue outside the window
      if (tid == 0) c.frame_flags[f] = 1u;
      return true;
    }
  }
  if (tid == 0) r->n_cluster = (int32_t)n;
  return true;
}

// ------------------------------------------------------------------ components on cells, the cells in a HASH TABLE (round 5)
// Frames the LDS cell grid cannot hold -- the un-cropped clouds of the online caller (get_chessboard_by_point,
// LidarCornersEst.cpp:72-115: a bounding grid of 1 269 x 1 720 x 249 cells against a 96 k-bit bitmap), or more occupied cells than
// the LDS arrays -- used to fall to the POINT-level spatial hash (every point against every point of 14 cells of side tol, chained
// buckets, device-scope atomics from many workgroups: 3.75 ms per 128 un-cropped VLP-16 clouds).  They now run the cell-level
// algorithm of fine_cluster_frame -- cells of side 0.57 tol are cliques, edges join occupied cells within +-2 per axis that hold a
// pair of points within tol -- with the dense bitmap replaced by an open-addressing hash table in global memory keyed by BLOCKS
// of 4 x 4 x 4 cells: an entry holds the block's 64-bit occupancy mask and the dense id of its first cell, so the 124-cell
// neighbourhood of a cell is read with at most 7 table lookups (the 2 x 2 x 2 blocks its 5-cell windows overlap, minus its own).
// The phases (hash_setup ... hash_tail) are written once and run by two callers, which differ in how they spread the work, what
// separates the phases, and the memory-scope policy they instantiate the phases with:
//   hashed_cluster_frame (WgScope): ONE workgroup per frame, and every atomic at WORKGROUP scope: on this part a device-scope
//     atomic or load is executed beyond the XCD's L2 (the L2s of the eight XCDs are not coherent with each other inside a kernel)
//     at several microseconds a piece -- measured here: 8 400 cycles per table lookup with device-scope loads, and a chain of
//     kernels over (frame, chunk) items with device-scope atomics took 2.7 ms for the same 128 clouds.  A frame's data is touched
//     by its own workgroup only, whose read-modify-writes then execute in the L2 of its XCD.  Plain loads may hit stale lines of
//     the CU's L1: every phase boundary (wg_phase) invalidates it (acquire fence), and inside a phase staleness is benign by
//     construction -- a table word goes from empty to a key once (a stale "empty" only costs a compare-and-swap that returns the
//     key), union-find parents only ever move to smaller indices (a stale parent is still an ancestor) and a failed hook
//     continues from the value the compare-and-swap returned.
//   the k2h_* chain (AgentScope, below): several workgroups share a frame, so atomics and the loads that race them are agent-scope.
// Scratch per frame (all dead at K2 time, rewritten by K3 / K4 / K5 / K5w / K7b afterwards): table keys = the frame's slice of
// uf_hash_head; base ids = board; masks = pca (low words) + optim (high words); per point / per cell words = uf_hash_next
// (cell of a point), uf_count (count, later component size), uf_parent (cell union-find), yz (smallest index | block-and-bit,
// later the root), walk_yz (sorted start).  Same cells, same pair arithmetic, same union rule, labels = smallest member index:
// the partition, the choice and the index-ordered output are those of the other paths (tests: the online caller, the wide sparse
// ROI and the large ROIs against the oracle's BFS).
constexpr uint32_t kHashEmpty = 0xFFFFFFFFu;
constexpr uint32_t kHashPointsMax = 65536u;            // frames above this keep the point-level path (table at most half full)
static_assert(2u * kHashPointsMax <= (uint32_t)kClusterHashSize, "hash table capacity");

constexpr uint32_t kHashMinFramePoints = 256;   // hashed-block path: 4 words per input point hold the smallest (1024-word) block table
struct HashFrame {
  float lox, loy, loz, inv;
  int32_t nbx, nby;       // blocks per axis (x, y); keys are bx + nbx * (by + nby * bz)
  uint32_t mask, shift;   // table size - 1, 32 - log2(size)
};
struct HashViews {
  const float4* P;
  float4* sorted;
  uint32_t *tkey, *tbase, *tlo, *thi;
  uint32_t *cell_of, *ccnt, *cpar, *cmin, *ckey, *cstart;
  uint32_t M;
};
__device__ __forceinline__ HashViews hash_views(const Ctx& c, uint32_t f) {
  const uint64_t beg = c.off[f];
  HashViews v;
  v.M = (uint32_t)c.res[f].n_roi;
  v.P = c.roi + beg;
  v.sorted = c.cluster + beg;
  v.tkey = c.uf_hash_head + (uint64_t)f * kClusterHashSize;
  v.tbase = reinterpret_cast<uint32_t*>(c.board + beg);
  v.tlo = reinterpret_cast<uint32_t*>(c.pca + beg);
  v.thi = reinterpret_cast<uint32_t*>(c.optim + beg);
  v.cell_of = c.uf_hash_next + beg;
  v.ccnt = c.uf_count + beg;
  v.cpar = c.uf_parent + beg;
  v.cmin = reinterpret_cast<uint32_t*>(c.yz + beg);
  v.ckey = v.cmin + v.M;
  v.cstart = reinterpret_cast<uint32_t*>(c.walk_yz + beg);   // M + 1 <= 2 M words
  return v;
}
__device__ __forceinline__ uint32_t hb_slot(const HashFrame& g, uint32_t key) { return (key * 0x9E3779B1u) >> g.shift; }
// block key and bit of a point's cell (cell coordinates + 2, as fine_key: neighbours never leave the padded grid)
__device__ __forceinline__ void hb_cell(const HashFrame& g, const float4& q, uint32_t& key, uint32_t& bit) {
  const int cx = (int)floorf((q.x - g.lox) * g.inv) + 2, cy = (int)floorf((q.y - g.loy) * g.inv) + 2,
            cz = (int)floorf((q.z - g.loz) * g.inv) + 2;
  key = (uint32_t)((cx >> 2) + g.nbx * ((cy >> 2) + g.nby * (cz >> 2)));
  bit = (uint32_t)((cx & 3) | ((cy & 3) << 2) | ((cz & 3) << 4));
}
__device__ __forceinline__ uint32_t hb_rank(uint32_t lo, uint32_t hi, uint32_t bit) {   // set bits below `bit`
  return bit < 32u ? (uint32_t)__popc(lo & ((1u << bit) - 1u)) : (uint32_t)__popc(lo) + (uint32_t)__popc(hi & ((1u << (bit - 32u)) - 1u));
}
__device__ __forceinline__ uint32_t hb_axis_mask(int a, int o) {   // cells x of block (own + o) with |x + 4 o - a| <= 2, as a 4-bit mask
  const int l = max(a - 2 - 4 * o, 0), u = min(a + 2 - 4 * o, 3);
  return l > u ? 0u : ((1u << (u + 1)) - 1u) & ~((1u << l) - 1u);
}
__device__ __forceinline__ uint32_t wg_cas(uint32_t* p, uint32_t expect, uint32_t desired) {
  __hip_atomic_compare_exchange_strong(p, &expect, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  return expect;   // the value found (== the `expect` passed in iff the exchange happened)
}
// phase boundary of a one-workgroup algorithm on global memory: everyone's stores and atomics are out, and nobody reads a stale L1 line
__device__ __forceinline__ void wg_phase() {
  __threadfence_block();
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // (buffer_inv: invalidates the CU's L1)
}
// -DILCC_K2_TIMING: counters of the one-workgroup path's edge search (union-find hops, cell pairs tested, thread-cycles per part)
struct NoClock {
  __device__ void lap(int) {}
  __device__ void pair() {}
  __device__ void hit() {}
  __device__ void flush() {}
};
#ifdef ILCC_K2_TIMING
__device__ unsigned long long g_k2_hops, g_k2_finds, g_k2_pairs, g_k2_hits, g_k2_t[6];
#define K2_COUNT(v, n) atomicAdd(&(v), (unsigned long long)(n))
struct EdgeClock {
  unsigned long long t[6] = {0, 0, 0, 0, 0, 0}, last = __builtin_readcyclecounter();
  __device__ void lap(int k) {
    const unsigned long long now = __builtin_readcyclecounter();
    t[k] += now - last;
    last = now;
  }
  __device__ void pair() { K2_COUNT(g_k2_pairs, 1); }
  __device__ void hit() { K2_COUNT(g_k2_hits, 1); }
  __device__ void flush() {
    for (int k = 0; k < 6; ++k) atomicAdd(&g_k2_t[k], t[k]);
  }
};
#else
#define K2_COUNT(v, n) do {} while (0)
using EdgeClock = NoClock;
#endif
// union-find on global parents owned by ONE workgroup: plain loads (a stale parent is still an ancestor: parents only move to
// smaller indices), hooks by workgroup-scope compare-and-swap; a failed hook continues from the parent the CAS returned
__device__ __forceinline__ uint32_t wg_find(uint32_t* parent, uint32_t x) {
  K2_COUNT(g_k2_finds, 1);
  for (;;) {
    K2_COUNT(g_k2_hops, 1);
    const uint32_t p = parent[x];
    if (p == x) return x;
    const uint32_t gp = parent[p];
    if (gp != p) parent[x] = gp;   // path halving (a non-root's word: hooks only ever touch roots)
    x = p;
  }
}
__device__ __forceinline__ void wg_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = wg_find(parent, a);
    b = wg_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = wg_cas(&parent[a], a, b);   // hook the larger root under the smaller one
    if (old == a) return;
    a = old;   // a was no root any more (our copy was stale): its real parent is smaller -- the loop terminates
  }
}

// The memory-scope policies the hashed phases are instantiated with: the scope of the read-modify-writes, the flavour of the
// loads that race them, the union-find, and the edge search's timing counters.
struct WgScope {   // hashed_cluster_frame: one workgroup owns the frame
  static constexpr int kScope = __HIP_MEMORY_SCOPE_WORKGROUP;
  using Clock = EdgeClock;
  static __device__ __forceinline__ uint32_t load(const uint32_t* p) { return *p; }
  static __device__ __forceinline__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t desired) { return wg_cas(p, expect, desired); }
  static __device__ __forceinline__ uint32_t find(uint32_t* parent, uint32_t x) { return wg_find(parent, x); }
  static __device__ __forceinline__ void unite(uint32_t* parent, uint32_t a, uint32_t b) { wg_unite(parent, a, b); }
};
struct AgentScope {   // the k2h_* chain: several workgroups share a frame
  static constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
  using Clock = NoClock;
  static __device__ __forceinline__ uint32_t load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t desired) { return atomicCAS(p, expect, desired); }
  static __device__ __forceinline__ uint32_t find(uint32_t* parent, uint32_t x) { return uf_find(parent, x); }
  static __device__ __forceinline__ void unite(uint32_t* parent, uint32_t a, uint32_t b) { uf_unite(parent, a, b); }
};
// a read-modify-write at the policy S's scope
#define HB_ATOMIC(op, ptr, val) __hip_atomic_##op((ptr), (val), __ATOMIC_RELAXED, S::kScope)
// ---- the phases.  Per frame: every thread of one workgroup calls them; per point / per cell: one thread per item.

// setup (per frame): bounding box -> block grid -> table size.  False (uniformly) when the frame is outside the hashed path's
// limits: its caller takes the point-level path.  scf: 112 floats.
__device__ __forceinline__ bool hash_setup(const Ctx& c, uint32_t f, const HashViews& v, float* scf, HashFrame& g) {
  const uint32_t M = v.M;
  // the block arrays (tbase / tlo / thi: at least 1024 words each) live in the frame's OWN slices of board / pca / optim, four
  // words per INPUT point: a frame of fewer than 256 input points cannot hold them (it wrote into its neighbour's)
  if (M == 0u || M > kHashPointsMax || c.off[f + 1] - c.off[f] < (uint64_t)kHashMinFramePoints) return false;
  float3 lo, hi;
  block_bbox(v.P, M, scf, lo, hi);
  g.lox = lo.x; g.loy = lo.y; g.loz = lo.z;
  g.inv = 1.0f / ((float)c.p.cluster_tol * kFineCellOverTol);
  const float ex = (hi.x - lo.x) * g.inv, ey = (hi.y - lo.y) * g.inv, ez = (hi.z - lo.z) * g.inv;
  if (!(ex < 8192.f && ey < 8192.f && ez < 8192.f)) return false;   // (also a NaN extent)
  const int nx = (int)floorf(ex) + 5, ny = (int)floorf(ey) + 5, nz = (int)floorf(ez) + 5;
  g.nbx = (nx + 3) >> 2;
  g.nby = (ny + 3) >> 2;
  // 32-bit keys, 0xFFFFFFFF = empty
  if ((unsigned long long)g.nbx * (unsigned long long)g.nby * (unsigned long long)((nz + 3) >> 2) >= 0xFFFFFFFFull) return false;
  uint32_t size = 1024u;
  while (size < 2u * M) size <<= 1;             // <= 2^17: blocks <= cells <= points, the table at most half full
  g.mask = size - 1u;
  g.shift = 32u - (uint32_t)__builtin_ctz(size);
  return true;
}

// reset (per frame): empty table, no cells; every cell its own union-find root
__device__ __forceinline__ void hash_reset(const HashViews& v, const HashFrame& g) {
  for (uint32_t k = threadIdx.x; k <= g.mask; k += blockDim.x) {
    v.tkey[k] = kHashEmpty;
    v.tlo[k] = 0u;
    v.thi[k] = 0u;
  }
  for (uint32_t i = threadIdx.x; i < v.M; i += blockDim.x) {
    v.ccnt[i] = 0u;
    v.cmin[i] = 0xFFFFFFFFu;
    v.cpar[i] = i;
  }
}

// insert (per point): its block's entry (claimed with a compare-and-swap on the key), its cell's bit
template <class S>
__device__ __forceinline__ void hash_insert(const HashViews& v, const HashFrame& g, uint32_t i) {
  uint32_t key, bit;
  hb_cell(g, v.P[i], key, bit);
  uint32_t h = hb_slot(g, key);
  for (;;) {
    uint32_t e = S::load(&v.tkey[h]);
    if (e == kHashEmpty) e = S::cas(&v.tkey[h], kHashEmpty, key);   // (a stale "empty" costs this CAS, which returns the key)
    if (e == kHashEmpty || e == key) break;
    h = (h + 1u) & g.mask;
  }
  HB_ATOMIC(fetch_or, bit < 32u ? &v.tlo[h] : &v.thi[h], 1u << (bit & 31u));
  v.cell_of[i] = (h << 6) | bit;
}

// block bases (per frame): first dense cell id of every block, an exclusive scan of the masks' popcounts (whole tiles of 4 slots
// per thread: the table size is a power of two >= 1024, 16-byte accesses).  Returns the number of cells.
__device__ __forceinline__ uint32_t hash_blocks(const HashViews& v, const HashFrame& g, uint32_t* sc) {
  const uint32_t size = g.mask + 1u;
  const uint4* lo4 = reinterpret_cast<const uint4*>(v.tlo);
  const uint4* hi4 = reinterpret_cast<const uint4*>(v.thi);
  uint4* base4 = reinterpret_cast<uint4*>(v.tbase);
  uint32_t C = 0;
  for (uint32_t t0 = 0; t0 < size / 4u; t0 += blockDim.x) {
    const uint32_t q = t0 + threadIdx.x;
    uint32_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;
    if (q < size / 4u) {
      const uint4 a = lo4[q], b = hi4[q];
      n0 = (uint32_t)(__popc(a.x) + __popc(b.x));
      n1 = (uint32_t)(__popc(a.y) + __popc(b.y));
      n2 = (uint32_t)(__popc(a.z) + __popc(b.z));
      n3 = (uint32_t)(__popc(a.w) + __popc(b.w));
    }
    uint32_t tot;
    const uint32_t run = C + block_excl_scan(n0 + n1 + n2 + n3, sc, tot);
    if (q < size / 4u) base4[q] = make_uint4(run, run + n0, run + n0 + n1, run + n0 + n1 + n2);
    C += tot;
  }
  return C;
}

// cells (per point): dense cell id (block's base + rank of the bit), cell count, smallest member index
template <class S>
__device__ __forceinline__ void hash_cell(const HashViews& v, uint32_t i) {
  const uint32_t hb = v.cell_of[i], h = hb >> 6, bit = hb & 63u;
  const uint32_t cell = v.tbase[h] + hb_rank(v.tlo[h], v.thi[h], bit);
  v.cell_of[i] = cell;
  HB_ATOMIC(fetch_add, &v.ccnt[cell], 1u);
  HB_ATOMIC(fetch_min, &v.cmin[cell], i);
  v.ckey[cell] = hb;   // (every point of the cell writes the same word)
}

// starts (per frame): first sorted position of every cell, an exclusive scan of the counts (tiles of one cell per thread: coalesced)
__device__ __forceinline__ void hash_starts(const HashViews& v, uint32_t C, uint32_t* sc) {
  uint32_t run0 = 0;
  for (uint32_t t0 = 0; t0 < C; t0 += blockDim.x) {
    const uint32_t k = t0 + threadIdx.x;
    const uint32_t n = k < C ? v.ccnt[k] : 0u;
    uint32_t tot;
    const uint32_t run = run0 + block_excl_scan(n, sc, tot);
    if (k < C) v.cstart[k] = run;
    run0 += tot;
  }
  if (threadIdx.x == 0) v.cstart[C] = v.M;
}

// place (per point): the points sorted by cell, in the frame's slice of the cluster buffer until the compaction (leaves the
// counts all zero)
template <class S>
__device__ __forceinline__ void hash_place(const HashViews& v, uint32_t i) {
  const uint32_t cell = v.cell_of[i];
  v.sorted[v.cstart[cell] + (HB_ATOMIC(fetch_sub, &v.ccnt[cell], 1u) - 1u)] = v.P[i];
}

// edges (per cell A): the occupied neighbour cells with a larger id; same root -> nothing; else the pair's points are tested
// until the first hit (the reference's float arithmetic) and the cells united (hooks to the smaller id)
template <class S>
__device__ __forceinline__ void hash_edges(const HashViews& v, const HashFrame& g, uint32_t A, float tol2, typename S::Clock& clk) {
  clk.lap(5);
  const uint32_t hb = v.ckey[A], hA = hb >> 6, bitA = hb & 63u;
  const uint32_t keyA = v.tkey[hA];
  const int ax = (int)(bitA & 3u), ay = (int)((bitA >> 2) & 3u), az = (int)(bitA >> 4);
  const uint32_t a0 = v.cstart[A], a1 = v.cstart[A + 1];
  // the 5-cell window of an axis overlaps the cell's own block and ONE neighbour: the lower one when the cell sits in the
  // block's lower half, the upper one otherwise
  const int sx = ax < 2 ? -1 : 1, sy = ay < 2 ? -1 : 1, sz = az < 2 ? -1 : 1;
  // slots first, then ALL first probes in flight at once, then all masks: no chain of dependent loads per neighbour
  uint32_t hs[8], want[8], got[8];
  hs[0] = hA;
#pragma unroll
  for (int nb = 1; nb < 8; ++nb) {
    const int ox = (nb & 1) ? sx : 0, oy = (nb & 2) ? sy : 0, oz = (nb & 4) ? sz : 0;
    want[nb] = (uint32_t)((int)keyA + ox + g.nbx * (oy + g.nby * oz));
    hs[nb] = hb_slot(g, want[nb]);
  }
#pragma unroll
  for (int nb = 1; nb < 8; ++nb) got[nb] = v.tkey[hs[nb]];
#pragma unroll
  for (int nb = 1; nb < 8; ++nb) {
    uint32_t h = hs[nb], e = got[nb];
    while (e != want[nb] && e != kHashEmpty) {   // (a collision: rare at <= 50 % load)
      h = (h + 1u) & g.mask;
      e = v.tkey[h];
    }
    hs[nb] = e == kHashEmpty ? kHashEmpty : h;
  }
  clk.lap(0);
  uint32_t mlo[8], mhi[8], base[8];
#pragma unroll
  for (int nb = 0; nb < 8; ++nb) {
    const uint32_t h = hs[nb] == kHashEmpty ? hA : hs[nb];   // (a harmless load for an absent block)
    mlo[nb] = v.tlo[h];
    mhi[nb] = v.thi[h];
    base[nb] = v.tbase[h];
  }
  uint32_t ra = S::find(v.cpar, A);
  clk.lap(1);
#pragma unroll
  for (int nb = 0; nb < 8; ++nb) {
    if (hs[nb] == kHashEmpty) continue;
    const int ox = (nb & 1) ? sx : 0, oy = (nb & 2) ? sy : 0, oz = (nb & 4) ? sz : 0;
    const uint32_t mx = hb_axis_mask(ax, ox), my = hb_axis_mask(ay, oy), mz = hb_axis_mask(az, oz);
    // window = { x + 4 y + 16 z : x in mx, y in my, z in mz }: products of disjoint bit patterns
    const uint32_t plane = mx * ((my & 1u) | ((my & 2u) << 3) | ((my & 4u) << 6) | ((my & 8u) << 9));   // 16 bits
    const unsigned long long win = (unsigned long long)plane *
                                   ((unsigned long long)(mz & 1u) | ((unsigned long long)(mz & 2u) << 15) | ((unsigned long long)(mz & 4u) << 30) | ((unsigned long long)(mz & 8u) << 45));
    unsigned long long occ = (((unsigned long long)mhi[nb] << 32) | mlo[nb]) & win;
    if (nb == 0) occ &= ~(1ull << bitA);
    while (occ) {
      const uint32_t b = (uint32_t)__builtin_ctzll(occ);
      occ &= occ - 1ull;
      const uint32_t B = base[nb] + hb_rank(mlo[nb], mhi[nb], b);
      if (B <= A) continue;   // every pair of cells once: from the smaller id
      clk.lap(2);
      const uint32_t rb = S::find(v.cpar, B);
      clk.lap(3);
      if (ra == rb) continue;   // (a stale ra only costs a redundant test: unite finds the roots itself)
      clk.pair();
      const uint32_t b0 = v.cstart[B], b1 = v.cstart[B + 1];
      // B's points four at a time (independent loads: one memory round trip per four), A's points inside (re-read for every
      // neighbour: L1 hits).  A serial walk over B's points for every point of A -- dense cells near the sensor hold dozens, and
      // two rings a cell apart never touch -- was most of this phase: one round trip per TEST, in the slowest lane of the wavefront
      bool hit = false;
      for (uint32_t ib = b0; ib < b1 && !hit; ib += 4u) {
        float4 q[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) q[k] = v.sorted[min(ib + k, b1 - 1u)];   // (the last point again past the end: harmless)
        for (uint32_t ia = a0; ia < a1 && !hit; ++ia) {
          const float4 pa = v.sorted[ia];
#pragma unroll
          for (uint32_t k = 0; k < 4u; ++k) {
            const float ex2 = q[k].x - pa.x, ey2 = q[k].y - pa.y, ez2 = q[k].z - pa.z;
            float d2 = ex2 * ex2;
            d2 = d2 + ey2 * ey2;
            d2 = d2 + ez2 * ez2;
            hit |= d2 < tol2;
          }
        }
      }
      clk.lap(4);
      if (hit) {
        clk.hit();
        S::unite(v.cpar, ra, rb);
        ra = S::find(v.cpar, A);
      }
      clk.lap(3);
    }
  }
}

// root (per cell A, its root found by the caller): kept in ckey (block-and-bit is no longer needed); size and smallest member
// index accumulated on the root (the counts are zero since the placement; a non-root's word is final since the cells phase)
template <class S>
__device__ __forceinline__ void hash_root(const HashViews& v, uint32_t A, uint32_t root) {
  v.ckey[A] = root;
  HB_ATOMIC(fetch_add, &v.ccnt[root], v.cstart[A + 1] - v.cstart[A]);
  if (root != A) HB_ATOMIC(fetch_min, &v.cmin[root], S::load(&v.cmin[A]));
}

// tail (per frame): components = the root cells, a point's = its cell's root
__device__ __forceinline__ void hash_tail(const Ctx& c, uint32_t f, const HashViews& v, uint32_t C, uint32_t* sc) {
  cluster_tail(c, f, v.P, v.M, C,
               [&](uint32_t k, uint32_t& sz, uint32_t& mi) {
                 if (v.ckey[k] != k) return false;
                 sz = v.ccnt[k];
                 mi = v.cmin[k];
                 return true;
               },
               [&](uint32_t i, const float4&) { return v.ckey[v.cell_of[i]]; }, sc);
}
// The phases by the frame's own workgroup.  Returns false (uniformly) when the frame is outside this path's limits: the caller
// takes the point-level path.
__device__ bool hashed_cluster_frame(const Ctx& c, uint32_t f, uint32_t* sc) {
  const HashViews v = hash_views(c, f);
  const uint32_t M = v.M, tid = threadIdx.x, kT = blockDim.x;
#ifdef ILCC_K2_TIMING
  __shared__ unsigned long long hmark[12];
#define HC_MARK(k) do { __syncthreads(); if (threadIdx.x == 0) hmark[k] = __builtin_readcyclecounter(); } while (0)
#else
#define HC_MARK(k) do {} while (0)
#endif
  HC_MARK(0);
  HashFrame g;
  if (!hash_setup(c, f, v, reinterpret_cast<float*>(sc), g)) return false;
  HC_MARK(1);
  hash_reset(v, g);
  wg_phase();
  HC_MARK(2);
  for (uint32_t i = tid; i < M; i += kT) hash_insert<WgScope>(v, g, i);
  wg_phase();
  HC_MARK(3);
  const uint32_t C = hash_blocks(v, g, sc);
  wg_phase();
  HC_MARK(4);
  for (uint32_t i = tid; i < M; i += kT) hash_cell<WgScope>(v, i);
  wg_phase();
  HC_MARK(5);
  hash_starts(v, C, sc);
  wg_phase();
  for (uint32_t i = tid; i < M; i += kT) hash_place<WgScope>(v, i);
  wg_phase();
  HC_MARK(6);
  {
    const float tol2 = (float)(c.p.cluster_tol * c.p.cluster_tol);
    WgScope::Clock clk;
    for (uint32_t A = tid; A < C; A += kT) hash_edges<WgScope>(v, g, A, tol2, clk);
    clk.flush();
  }
  wg_phase();
  HC_MARK(7);
  for (uint32_t t0 = 0; t0 < C; t0 += kT) {
    const uint32_t A = t0 + tid;
    uint32_t root = 0;
    if (A < C) root = wg_find(v.cpar, A);
    wg_phase();   // (path halving rewrites parents: finish every find of the tile before the roots are stored)
    if (A < C) hash_root<WgScope>(v, A, root);
  }
  wg_phase();
  HC_MARK(8);
  hash_tail(c, f, v, C, sc);
  HC_MARK(9);
#ifdef ILCC_K2_TIMING
  if (tid == 0)
    printf("K2 counters (all frames so far): finds %llu hops %llu cell pairs tested %llu hits %llu; thread-cycles lookups %llu masks+findA %llu window %llu find/unite %llu tests %llu loop %llu\n", g_k2_finds, g_k2_hops, g_k2_pairs, g_k2_hits, g_k2_t[0], g_k2_t[1], g_k2_t[2], g_k2_t[3], g_k2_t[4], g_k2_t[5]);
  if (tid == 0)
    printf("K2 hashed M=%u C=%u table %u cycles: bbox %llu reset %llu insert %llu blocks %llu cells %llu sort %llu edges %llu comps %llu nn+compact %llu\n",
           M, C, g.mask + 1u, hmark[1] - hmark[0], hmark[2] - hmark[1], hmark[3] - hmark[2], hmark[4] - hmark[3], hmark[5] - hmark[4], hmark[6] - hmark[5],
           hmark[7] - hmark[6], hmark[8] - hmark[7], hmark[9] - hmark[8]);
#endif
  return true;
}

// ------------------------------------------------------------------ the same components, the whole chip on a few frames
// k2h_*: the second tier of the online caller (get_chessboard_by_point on un-cropped clouds, LidarCornersEst.cpp:72-115).  The
// first tier answers most frames from a window; the few it cannot vouch for -- listed in Ctx::list -- need the WHOLE cloud
// clustered, ~29 k points and ~20 k cells each.  One workgroup per frame (hashed_cluster_frame) is latency-bound there: every
// phase is a few dozen dependent memory round trips per thread, 2.1 ms per frame however few frames there are.  This chain of
// kernels runs the same phases, one kernel each, with the per-point and per-cell ones spread over (listed frame, 256-item chunk)
// work items on the whole chip; its atomics are agent-scope (AgentScope: several workgroups share a frame) and therefore slow
// one by one -- 2.7 ms when all 128 clouds of a call are listed -- but with a tenth of the frames listed the chain is a tenth
// as long.
//   k2h_setup   per frame: hash_setup, hash_reset        k2h_starts  per frame: hash_starts
//   k2h_insert  per point: hash_insert                   k2h_place   per point: hash_place
//   k2h_blocks  per frame: hash_blocks                   k2h_edges   per cell:  hash_edges
//   k2h_cells   per point: hash_cell                     k2h_roots   per cell:  its root, hash_root
//   k2h_finish  per frame: hash_tail (point_level_cluster_frame for a frame outside the hashed path's limits)
// Same scratch as hashed_cluster_frame (hash_views).
constexpr int kListChunk = 256;       // items per work item
constexpr int kListBlock = 1024;      // listed frames whose chunk prefix sums a workgroup keeps in LDS at a time
struct ListedFrame {   // per frame (indexed by frame, valid for listed frames)
  HashFrame g;
  uint32_t n_cells;
  uint32_t valid;      // 0: outside the hashed path's limits: k2h_finish clusters the frame with the point-level search
  uint32_t pad[6];
};
static_assert(sizeof(ListedFrame) == 64, "ilcc_api.cpp allocates 64 bytes per frame");

// calls fn(f, first item of the chunk) for this workgroup's share of the (listed frame, chunk of kListChunk items) work items;
// count(f) = the frame's items (points, or cells).  Every thread of the workgroup makes the same calls.
template <typename Count, typename Fn>
__device__ __forceinline__ void for_each_listed_chunk(const Ctx& c, uint32_t* s_pref, Count count, Fn fn) {
  const uint32_t nl = __hip_atomic_load(c.list_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (uint32_t base = 0; base < nl; base += kListBlock) {
    const uint32_t nb = min((uint32_t)kListBlock, nl - base);
    __syncthreads();
    // chunks per listed frame, read in parallel, then an inclusive scan by the first wavefront: s_pref[j] = chunks of the frames before j
    for (uint32_t j = threadIdx.x; j < nb; j += blockDim.x) s_pref[j + 1] = (count(c.list[base + j]) + kListChunk - 1) / kListChunk;
    if (threadIdx.x == 0) s_pref[0] = 0u;
    __syncthreads();
    if (wave_id() == 0) {
      const uint32_t per = (nb + ILCC_WAVE - 1u) / ILCC_WAVE, k0 = min(nb + 1u, 1u + (uint32_t)lane_id() * per), k1 = min(nb + 1u, k0 + per);
      uint32_t sum = 0;
      for (uint32_t k = k0; k < k1; ++k) sum += s_pref[k];
      uint32_t incl = sum;
#pragma unroll
      for (int o = 1; o < ILCC_WAVE; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o, ILCC_WAVE);
        if (lane_id() >= o) incl += t;
      }
      uint32_t run = incl - sum;
      for (uint32_t k = k0; k < k1; ++k) {
        run += s_pref[k];
        s_pref[k] = run;
      }
    }
    __syncthreads();
    const uint32_t total = s_pref[nb];
    for (uint32_t item = blockIdx.x; item < total; item += gridDim.x) {
      uint32_t lo = 0, hi = nb;   // last j with s_pref[j] <= item
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_pref[mid] <= item) lo = mid; else hi = mid;
      }
      fn(c.list[base + lo], (item - s_pref[lo]) * kListChunk);
    }
  }
}

// the listed frame of this workgroup, for the per-frame kernels (one workgroup per listed frame)
__device__ __forceinline__ bool listed_frame(const Ctx& c, uint32_t& f) {
  if (blockIdx.x >= __hip_atomic_load(c.list_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;
  f = c.list[blockIdx.x];
  return true;
}

__global__ __launch_bounds__(1024) void k2h_setup(Ctx c, ListedFrame* frames) {
  __shared__ float scf[128];
  uint32_t f;
  if (!listed_frame(c, f)) return;
  const HashViews v = hash_views(c, f);
  HashFrame g{};
  const bool ok = hash_setup(c, f, v, scf, g);
  if (threadIdx.x == 0) {
    ListedFrame L{};   // (valid = 0: n_cells = 0)
    L.g = g;
    L.valid = ok ? 1u : 0u;
    frames[f] = L;
  }
  if (ok) hash_reset(v, g);
}

__global__ __launch_bounds__(kListChunk) void k2h_insert(Ctx c, const ListedFrame* frames) {
  __shared__ uint32_t s_pref[kListBlock + 1];
  for_each_listed_chunk(c, s_pref, [&](uint32_t f) { return frames[f].valid ? (uint32_t)c.res[f].n_roi : 0u; }, [&](uint32_t f, uint32_t first) {
    const HashViews v = hash_views(c, f);
    const uint32_t i = first + threadIdx.x;
    if (i < v.M) hash_insert<AgentScope>(v, frames[f].g, i);
  });
}

__global__ __launch_bounds__(1024) void k2h_blocks(Ctx c, ListedFrame* frames) {
  __shared__ uint32_t sc[32];
  uint32_t f;
  if (!listed_frame(c, f) || !frames[f].valid) return;
  const uint32_t C = hash_blocks(hash_views(c, f), frames[f].g, sc);
  if (threadIdx.x == 0) frames[f].n_cells = C;
}

__global__ __launch_bounds__(kListChunk) void k2h_cells(Ctx c, const ListedFrame* frames) {
  __shared__ uint32_t s_pref[kListBlock + 1];
  for_each_listed_chunk(c, s_pref, [&](uint32_t f) { return frames[f].valid ? (uint32_t)c.res[f].n_roi : 0u; }, [&](uint32_t f, uint32_t first) {
    const HashViews v = hash_views(c, f);
    const uint32_t i = first + threadIdx.x;
    if (i < v.M) hash_cell<AgentScope>(v, i);
  });
}

__global__ __launch_bounds__(1024) void k2h_starts(Ctx c, const ListedFrame* frames) {
  __shared__ uint32_t sc[32];
  uint32_t f;
  if (!listed_frame(c, f) || !frames[f].valid) return;
  hash_starts(hash_views(c, f), frames[f].n_cells, sc);
}

__global__ __launch_bounds__(kListChunk) void k2h_place(Ctx c, const ListedFrame* frames) {
  __shared__ uint32_t s_pref[kListBlock + 1];
  for_each_listed_chunk(c, s_pref, [&](uint32_t f) { return frames[f].valid ? (uint32_t)c.res[f].n_roi : 0u; }, [&](uint32_t f, uint32_t first) {
    const HashViews v = hash_views(c, f);
    const uint32_t i = first + threadIdx.x;
    if (i < v.M) hash_place<AgentScope>(v, i);
  });
}

__global__ __launch_bounds__(kListChunk) void k2h_edges(Ctx c, const ListedFrame* frames) {
  __shared__ uint32_t s_pref[kListBlock + 1];
  const float tol2 = (float)(c.p.cluster_tol * c.p.cluster_tol);
  for_each_listed_chunk(c, s_pref, [&](uint32_t f) { return frames[f].n_cells; }, [&](uint32_t f, uint32_t first) {
    const uint32_t A = first + threadIdx.x;
    if (A >= frames[f].n_cells) return;
    AgentScope::Clock clk;
    hash_edges<AgentScope>(hash_views(c, f), frames[f].g, A, tol2, clk);
  });
}

__global__ __launch_bounds__(kListChunk) void k2h_roots(Ctx c, const ListedFrame* frames) {
  __shared__ uint32_t s_pref[kListBlock + 1];
  for_each_listed_chunk(c, s_pref, [&](uint32_t f) { return frames[f].n_cells; }, [&](uint32_t f, uint32_t first) {
    const uint32_t A = first + threadIdx.x;
    if (A >= frames[f].n_cells) return;
    const HashViews v = hash_views(c, f);
    hash_root<AgentScope>(v, A, uf_find(v.cpar, A));
  });
}

__global__ __launch_bounds__(1024) void k2h_finish(Ctx c, const ListedFrame* frames) {
  __shared__ uint32_t sc[160];
  uint32_t f;
  if (!listed_frame(c, f)) return;
  const HashViews v = hash_views(c, f);
  if (!frames[f].valid) {   // beyond the hashed path's limits (> 65 536 points, a bounding grid of > 2^32 blocks): point-level search
    point_level_cluster_frame(c, f, sc);
    return;
  }
  hash_tail(c, f, v, frames[f].n_cells, sc);
}

// second tier of the online caller: the flagged frames, listed (one thread per frame: a few dozen frames at most matter)
__global__ __launch_bounds__(256) void k2h_list(Ctx c) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < c.n_frames && c.frame_flags[f] != 0u && c.res[f].status == ILCC_OK) c.list[atomicAdd(c.list_count, 1u)] = f;
}

uint32_t cluster_bits_default() { return (uint32_t)kFineBits; }
uint32_t cluster_bits_online() { return (uint32_t)kFineBitsOnline; }
size_t cluster_lds_bytes(uint32_t pts_cap, uint32_t cells_cap, uint32_t bits) {
  return 160 * sizeof(uint32_t) + sizeof(uint32_t) * fine_words(bits) + sizeof(uint16_t) * (bits / 64) +
         sizeof(uint32_t) * (5 * (size_t)cells_cap + 2) + 3 * sizeof(float) * (size_t)pts_cap;
}

__global__ __launch_bounds__(1024) void k2_seeded_cluster(Ctx c) {
  extern __shared__ __align__(16) unsigned char smem[];
  FineLds L;
  L.sc = reinterpret_cast<uint32_t*>(smem);                  // 160 words
  L.bm = L.sc + 160;                                        // 8-byte aligned: read as 64-bit words, too
  L.pre = reinterpret_cast<uint16_t*>(L.bm + fine_words(c.cluster_bits));
  const uint32_t cc = c.cluster_cells_cap;
  L.ckey = reinterpret_cast<uint32_t*>(L.pre + c.cluster_bits / 64);
  L.cstart = L.ckey + cc;
  L.ccnt = L.cstart + cc + 2;
  L.cmin = L.ccnt + cc;
  L.cpar = L.cmin + cc;
  L.sx = reinterpret_cast<float*>(L.cpar + cc);
  L.sy = L.sx + c.cluster_lds_points;
  L.sz = L.sy + c.cluster_lds_points;
  const uint32_t f = blockIdx.x;
  if (c.res[f].status != ILCC_OK) return;
  // first tier of the online caller: frames K1 has already handed on (empty window) are the second tier's
  if (c.online_tier == 1u && c.frame_flags[f] != 0u) return;
  const uint32_t M = (uint32_t)c.res[f].n_roi;
  const bool done = (M <= c.cluster_lds_points) ? fine_cluster_frame<true>(c, f, L) : fine_cluster_frame<false>(c, f, L);
  if (done) return;
  if (c.online_tier == 1u) {   // the window's points do not fit the LDS grid (capacity): the second tier clusters the whole cloud
    if (threadIdx.x == 0) c.frame_flags[f] = 1u;
    return;
  }
  // the LDS cell grid cannot hold this frame: the same components on cells with the cells in a hash table (global memory) ...
  __syncthreads();
  if (hashed_cluster_frame(c, f, L.sc)) return;
  // ... and beyond that path's limits (> 65 536 ROI points in one frame, a bounding grid of > 2^32 blocks): point-level search
  __syncthreads();
  point_level_cluster_frame(c, f, L.sc);
}

// up to a CU's whole LDS as dynamic LDS (> the 64 KiB default cap).  Called by ilcc_create for the handle's device: the attribute
// is kept per (function, device).
hipError_t set_kernel_attributes_k2() {
#ifdef ILCC_K2_TIMING
  return hipFuncSetAttribute((const void*)k2_seeded_cluster, hipFuncAttributeMaxDynamicSharedMemorySize, kClusterLdsMax);   // (the timers' static LDS)
#else
  return hipFuncSetAttribute((const void*)k2_seeded_cluster, hipFuncAttributeMaxDynamicSharedMemorySize, kCuLdsBytes);
#endif
}

hipError_t cluster_limits(int device, ClusterLimits* out) {
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) return e;
  hipFuncAttributes attr;
  if ((e = hipFuncGetAttributes(&attr, (const void*)k2_seeded_cluster)) != hipSuccess) return e;
  out->cus = (uint32_t)std::max(prop.multiProcessorCount, 1);
  out->lds_per_cu = (uint32_t)prop.maxSharedMemoryPerMultiProcessor;
  out->threads_per_cu = (uint32_t)std::max(prop.maxThreadsPerMultiProcessor, 1024);
  out->static_lds = (uint32_t)attr.sharedSizeBytes;
  return hipSuccess;
}

// frames (= workgroups) of one K2 launch the device holds at once, by LDS and by thread slots
static uint32_t cluster_resident_frames(const ClusterLimits& lim, uint32_t threads, size_t dynamic_lds) {
  const size_t per_wg = (size_t)lim.static_lds + dynamic_lds;
  const uint32_t by_lds = (uint32_t)((size_t)lim.lds_per_cu / std::max<size_t>(per_wg, 1)), by_threads = lim.threads_per_cu / threads;
  return lim.cus * std::min(by_lds, by_threads);
}

// The home of the cell-sorted points, per launch.  A workgroup's latency chain is about the same length wherever its pair tests
// read from (they load B's points in groups); what the LDS copy costs is residency: 12 bytes per point of capacity, half the
// footprint at the bench's (1792, 2560) reservation -- two workgroups per CU instead of four, and a 1024-frame batch in two rounds
// of one frame's chain.  So: LDS while every frame of the batch is resident at once even with the copy; otherwise no copy -- every
// frame takes fine_cluster_frame<false>, the path of frames above the capacity, the points in the frame's slice of `cluster` (L2).
// The online caller's first tier (wide) keeps LDS: a synchronous call on windows of a few hundred points.
ClusterLaunch launch_cluster(const Ctx& c, hipStream_t s, const ClusterLimits& lim, int32_t home) {
  if (c.online_tier == 2u) {   // the frames the online caller's first tier could not vouch for: the k2h_* chain over the listed frames
    ListedFrame* lf = static_cast<ListedFrame*>(c.list_frames);
    const uint32_t grid = c.list_grid;
    (void)hipMemsetAsync(c.list_count, 0, sizeof(uint32_t), s);
    hipLaunchKernelGGL(k2h_list, dim3((c.n_frames + 255u) / 256u), dim3(256), 0, s, c);
    hipLaunchKernelGGL(k2h_setup, dim3(c.n_frames), dim3(1024), 0, s, c, lf);
    hipLaunchKernelGGL(k2h_insert, dim3(grid), dim3(kListChunk), 0, s, c, lf);
    hipLaunchKernelGGL(k2h_blocks, dim3(c.n_frames), dim3(1024), 0, s, c, lf);
    hipLaunchKernelGGL(k2h_cells, dim3(grid), dim3(kListChunk), 0, s, c, lf);
    hipLaunchKernelGGL(k2h_starts, dim3(c.n_frames), dim3(1024), 0, s, c, lf);
    hipLaunchKernelGGL(k2h_place, dim3(grid), dim3(kListChunk), 0, s, c, lf);
    hipLaunchKernelGGL(k2h_edges, dim3(grid), dim3(kListChunk), 0, s, c, lf);
    hipLaunchKernelGGL(k2h_roots, dim3(grid), dim3(kListChunk), 0, s, c, lf);
    hipLaunchKernelGGL(k2h_finish, dim3(c.n_frames), dim3(1024), 0, s, c, lf);
    return ClusterLaunch{};
  }
  const int threads = (c.n_frames <= (uint32_t)kSmallBatchFrames || c.wide) ? 1024 : kFrameThreads;   // (small batches: latency, not CU footprint, matters)
  const size_t with_copy = cluster_lds_bytes(c.cluster_lds_points, c.cluster_cells_cap, c.cluster_bits);
  if (home == kClusterHomeRule)
    home = (c.wide || c.n_frames <= cluster_resident_frames(lim, (uint32_t)threads, with_copy)) ? kClusterHomeLds : kClusterHomeL2;
  Ctx k = c;
  if (home == kClusterHomeL2) k.cluster_lds_points = 0u;   // no frame fits "the capacity": fine_cluster_frame<false> for all
  const size_t lds = cluster_lds_bytes(k.cluster_lds_points, k.cluster_cells_cap, k.cluster_bits);
  hipLaunchKernelGGL(k2_seeded_cluster, dim3(k.n_frames), dim3(threads), lds, s, k);
  return ClusterLaunch{home, (uint32_t)lds, (uint32_t)threads};
}

}  // namespace ilcc
