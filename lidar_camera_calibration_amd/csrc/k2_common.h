// K2 seeded_cluster -- replaces pcl::EuclideanClusterExtraction + nearestKSearch of
// LidarCornersEst::EuclideanCluster (ilcc2/src/LidarCornersEst.cpp:124-153).
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
//
// The files: k2_cluster.hip (the per-frame launch k2_seeded_cluster: the LDS-grid path, the list of the frames it cannot hold,
// the launcher), k2_fallback.hip (k2_fallback_cluster behind it: a listed frame's hashed cells by one workgroup, the point-level
// search), k2h_listed.hip (the k2h_* chain and its launcher), k2_hashed.h (the hashed-cell phases those two run),
// k2_point_level.h (the last resort of both) and this header: the union-find, the block-wide helpers, the reference's distance
// and the tail every path ends in.  Included by the three .hip files (the last two through k2_hashed.h and k2_point_level.h).
#pragma once

#include "ilcc_internal.h"

namespace ilcc {

constexpr float kFineCellOverTol = 0.57f;        // s / tol: 3 s^2 = 0.9747 tol^2 < tol^2 (cell = clique), tol / s = 1.754 < 2 (neighbours within +-2 cells)

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

// Squared length of a difference of two points as the reference computes it: float, one product and one sum at a time, nothing
// fused (an -O3 x86-64 PCL / FLANN build contracts no multiply-add; the K2 files are built with -ffp-contract=off).  Every
// radius test compares it with FLANN's strict `<` against (float)(tol * tol); the click's 1-NN is its smallest value.
__device__ __forceinline__ float ref_dist2(float ex, float ey, float ez) {
  float d2 = ex * ex;
  d2 = d2 + ey * ey;
  d2 = d2 + ez * ez;
  return d2;
}

struct NnKey {
  float d2;
  uint32_t idx;
};
__device__ __forceinline__ bool nn_less(const NnKey& x, const NnKey& y) {
  return x.d2 < y.d2 || (x.d2 == y.d2 && x.idx < y.idx);
}

// ------------------------------------------------------------------ block-wide helpers
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

// ------------------------------------------------------------------ the tail of every path
// On the components k < n_comp of a frame's points P[0, M): comp(k, size, min_index) is true when k is
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
    const NnKey k{ref_dist2(q.x - click.x, q.y - click.y, q.z - click.z), i};
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

}  // namespace ilcc
