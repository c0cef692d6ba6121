// K15 seed_components -- where could the chessboard be?  (include/ilcc_seed.h states what is computed; this file how.)
//
// Voxel components of a whole scan and their exact second moments: occupied cells of edge >= the clustering tolerance go into a
// per-frame hash set, union-find joins 26-adjacent cells, and every component's n, sum q, sum q q^T are accumulated as int64.
// All deciding arithmetic is integer, so no result depends on the order in which threads run; only ordinary vector atomics and
// vector stores are used, and no workgroup waits for another (a failed compare-and-swap means another thread's succeeded).
//
// Six launches per batch, every one over a grid of (blocks, frames):
//   clear     the hash sets' keys and the per-frame counters (the caller's scratch arrives in any state)
//   insert    one point per lane, 16 B float4 loads in input order (a wavefront reads 1 KiB contiguous, like K1's count pass):
//             quantise, key, insert.  The lane that claims a slot numbers the cell and zeroes its moments
//   moments   the same read a second time: key, look-up, 10 int64 atomic adds on the point's CELL (a few points per cell -- adding
//             to the component's root at once would serialise a ground plane's thousands of points on ten addresses); lanes of one
//             ring at neighbouring azimuths are folded into one first
//   union     one lane per cell: 13 forward neighbours looked up in the set, found ones united (root = smallest key)
//   reduce    one lane per cell: a cell that is not its component's root adds its moments to the root's, a wavefront's cells of one
//             root as one sum
//   pack      one lane per cell: a root of n >= cluster_min claims a record
// Planar seeds (K15p; a set SeedCtx::core selects them): a `classify` launch between moments and union flags the cells whose
// 3 x 3 x 3 block is one flat two-dimensional patch that the cell's own points lie in (CORE cells), and union, reduce and pack
// then form the components of the core cells alone -- a board standing on the floor or on a pole is cut from them where the
// blocks hold two surfaces or a line.  The same properties hold: every loop has a stated bound, no workgroup waits for another,
// only ordinary vector atomics and vector stores are used, and the flag is a pure function of exact integer sums (one conversion
// to fp64 each, then unfused IEEE + - x / sqrt in a fixed order), so nothing decided depends on thread order.
//   classify  one lane per cell: 27 look-ups, up to 270 int64 loads (L2-resident), the block's covariance in int64, one
//             thread-serial Jacobi (eig3.h), three comparisons, one byte stored.  Block sum and eigen-solve share the kernel: the
//             sums are dead once the six covariance entries are converted, so they do not add to the solver's registers
// The passes over points are HBM-bound (16 B read per point each, plus the set's traffic in L2); the passes over cells touch a
// fraction of that.  They are separate launches because each needs the one before it complete for the whole frame.
#include <hip/hip_runtime.h>

#include "eig3.h"
#include "k15_seed.h"

namespace ilcc {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t ld(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// quantise one coordinate: false = dropped (non-finite, or beyond range_q).  v * 1024 is exact in fp32 (or overflows to an
// infinity, which the range test drops); this file is built with -ffp-contract=off, so the sum is the fp32 sum
__device__ __forceinline__ bool quantise(float v, int32_t range_q, int32_t* q) {
  const float t = floorf(v * 1024.0f + 0.5f);
  if (!(fabsf(t) <= (float)range_q)) return false;   // NaN fails too
  *q = (int32_t)t;
  return true;
}

__device__ __forceinline__ int32_t floor_div(int32_t q, int32_t d) { return q >= 0 ? q / d : -((-q + d - 1) / d); }

// the point's cell key, or false when the point is dropped
__device__ __forceinline__ bool point_key(const float4 p, const SeedGrid& g, int32_t q[3], uint32_t* key) {
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) return false;
  if (!quantise(p.x, g.range_q, &q[0]) || !quantise(p.y, g.range_q, &q[1]) || !quantise(p.z, g.range_q, &q[2])) return false;
  const int32_t ix = floor_div(q[0], g.cq) + g.off, iy = floor_div(q[1], g.cq) + g.off, iz = floor_div(q[2], g.cq) + g.off;
  *key = (uint32_t)(ix + g.N * (iy + g.N * iz));   // 0 <= ix, iy, iz < N <= 1024 since |q| <= range_q <= off cq
  return true;
}

__device__ __forceinline__ float4 load_point(const float4* src) {
  const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src));
  return make_float4(v.x, v.y, v.z, v.w);
}

// slot of `key` in the frame's set, or kSeedEmpty when the cell is not occupied.  Read-only: for launches behind the insert
__device__ __forceinline__ uint32_t find_slot(const uint32_t* tab, const SeedFrame& fr, uint32_t key) {
  uint32_t slot = (key * 2654435761u) >> fr.tab_shift;
  // at most tab_mask + 1 probes: the set has >= 2 n slots for <= n keys, so a free slot ends every probe sequence
  for (uint32_t probe = 0; probe <= fr.tab_mask; ++probe) {
    const uint32_t k = tab[slot];
    if (k == key) return slot;
    if (k == kSeedEmpty) return kSeedEmpty;
    slot = (slot + 1u) & fr.tab_mask;
  }
  return kSeedEmpty;
}

__global__ __launch_bounds__(kSeedThreads) void k15_clear(SeedCtx c) {
  const uint64_t stride = (uint64_t)gridDim.x * kSeedThreads;
  // ceil(slots_total / stride) trips
  for (uint64_t i = (uint64_t)blockIdx.x * kSeedThreads + threadIdx.x; i < c.slots_total; i += stride) {
    c.tab_key[i] = kSeedEmpty;
    if (i < 2ull * c.n_frames) c.counters[i] = 0u;   // (slots_total >= 64 n_frames)
  }
}

__global__ __launch_bounds__(kSeedThreads) void k15_insert(SeedCtx c) {
  const uint32_t f = blockIdx.y;
  const SeedFrame fr = c.fr[f];
  uint32_t* tab = c.tab_key + fr.tab_beg;
  const uint32_t stride = gridDim.x * kSeedThreads;
  // ceil(n / stride) trips
  for (uint32_t i = blockIdx.x * kSeedThreads + threadIdx.x; i < fr.n; i += stride) {
    const float4 p = load_point(c.xyzi + fr.pt_beg + i);
    int32_t q[3];
    uint32_t key;
    if (!point_key(p, c.g, q, &key)) continue;
    uint32_t slot = (key * 2654435761u) >> fr.tab_shift;
    // at most tab_mask + 1 probes: >= 2 n slots for <= n keys, a slot once taken keeps its key
    for (uint32_t probe = 0; probe <= fr.tab_mask; ++probe) {
      uint32_t k = ld(&tab[slot]);
      if (k == kSeedEmpty) k = atomicCAS(&tab[slot], kSeedEmpty, key);
      if (k == kSeedEmpty) {   // this lane claimed the slot: it numbers the cell (nothing reads the number before the next launch)
        const uint32_t ord = atomicAdd(&c.counters[2 * f], 1u);
        const uint64_t cell = fr.pt_beg + ord;   // cells <= points: the frame's point range holds them
        c.tab_ord[fr.tab_beg + slot] = ord;
        c.cell_key[cell] = key;
        c.parent[cell] = ord;
#pragma unroll
        for (int m = 0; m < kSeedMoments; ++m) c.mom[cell * kSeedMoments + m] = 0;
        break;
      }
      if (k == key) break;
      slot = (slot + 1u) & fr.tab_mask;
    }
  }
}

__device__ __forceinline__ void add64(long long* p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);   // two's complement: the sum is the signed sum
}

constexpr uint32_t kNoCell = 0xFFFFFFFFu;

__global__ __launch_bounds__(kSeedThreads) void k15_moments(SeedCtx c) {
  const uint32_t f = blockIdx.y;
  const SeedFrame fr = c.fr[f];
  const uint32_t* tab = c.tab_key + fr.tab_beg;
  const uint32_t stride = gridDim.x * kSeedThreads;
  const int lane = threadIdx.x & 63;
  // ceil(n / stride) trips, the same for every lane of the workgroup (the lanes exchange values below)
  for (uint32_t base = blockIdx.x * kSeedThreads; base < fr.n; base += stride) {
    const uint32_t i = base + threadIdx.x;
    int32_t q[3] = {0, 0, 0};
    uint32_t cell = kNoCell;   // the point's cell ordinal; kNoCell: no point, or a dropped one
    if (i < fr.n) {
      const float4 p = load_point(c.xyzi + fr.pt_beg + i);
      uint32_t key;
      if (point_key(p, c.g, q, &key)) {
        const uint32_t slot = find_slot(tab, fr, key);
        if (slot != kSeedEmpty) cell = c.tab_ord[fr.tab_beg + slot];   // (always found: the insert saw the same point)
      }
    }
    // |q| <= range_q <= 20 480 by default: a product is below 2^29, a frame of 2^17 points sums below 2^46; the host caps range_q at
    // sqrt(2^62 / max_total_points), so no sum leaves int64 for any batch the handle accepts
    const long long x = q[0], y = q[1], z = q[2];
    long long v[kSeedMoments] = {1, x, y, z, x * x, x * y, x * z, y * y, y * z, z * z};
    // A spinning LiDAR fires ring-minor: lanes l, l + 16, l + 32, l + 48 of a wavefront are the same ring at neighbouring azimuths --
    // a centimetre apart, mostly one cell.  Two exchange steps fold such lanes into one before the atomics (integer sums: exact in
    // any order); for any other input order they merely find fewer equal cells
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const uint32_t other = __shfl_xor(cell, off, 64);
      long long pv[kSeedMoments];
#pragma unroll
      for (int m = 0; m < kSeedMoments; ++m) pv[m] = __shfl_xor(v[m], off, 64);
      if (cell != kNoCell && other == cell) {
        if (lane & off) {
          cell = kNoCell;   // the lower lane of the pair carries both
        } else {
#pragma unroll
          for (int m = 0; m < kSeedMoments; ++m) v[m] += pv[m];
        }
      }
    }
    if (cell != kNoCell) {
      long long* dst = c.mom + (fr.pt_beg + cell) * kSeedMoments;
#pragma unroll
      for (int m = 0; m < kSeedMoments; ++m) add64(dst + m, v[m]);
    }
  }
}

// ---- K15p classify.  The order of every fp64 operation below is part of the specification (include/ilcc_seed.h, K15p);
// tests/seed_planar_ref.py restates it operation for operation.

// a cell's ten moments about the origin o (quanta): q' = q - o.  Unsigned arithmetic: exact modulo 2^64 whatever the size of the
// intermediate products, and the translated sums are small (|q'| <= 2 cq for every point of the block)
__device__ __forceinline__ void translate(const long long m[kSeedMoments], const long long o[3], long long t[kSeedMoments]) {
  typedef unsigned long long u64;
  const u64 n = (u64)m[0], ox = (u64)o[0], oy = (u64)o[1], oz = (u64)o[2];
  const u64 sx = (u64)m[1], sy = (u64)m[2], sz = (u64)m[3];
  t[0] = m[0];
  t[1] = (long long)(sx - n * ox);
  t[2] = (long long)(sy - n * oy);
  t[3] = (long long)(sz - n * oz);
  t[4] = (long long)((u64)m[4] - ox * sx - ox * sx + n * ox * ox);
  t[5] = (long long)((u64)m[5] - ox * sy - oy * sx + n * ox * oy);
  t[6] = (long long)((u64)m[6] - ox * sz - oz * sx + n * ox * oz);
  t[7] = (long long)((u64)m[7] - oy * sy - oy * sy + n * oy * oy);
  t[8] = (long long)((u64)m[8] - oy * sz - oz * sy + n * oy * oz);
  t[9] = (long long)((u64)m[9] - oz * sz - oz * sz + n * oz * oz);
}

__global__ __launch_bounds__(kSeedThreads) void k15_classify(SeedCtx c) {
  const uint32_t f = blockIdx.y;
  const SeedFrame fr = c.fr[f];
  const uint32_t n_cells = c.counters[2 * f];
  const uint32_t* tab = c.tab_key + fr.tab_beg;
  const int32_t N = c.g.N;
  const uint32_t stride = gridDim.x * kSeedThreads;
  // ceil(n_cells / stride) trips
  for (uint32_t i = blockIdx.x * kSeedThreads + threadIdx.x; i < n_cells; i += stride) {
    const uint32_t k = c.cell_key[fr.pt_beg + i];
    const int32_t ix = (int32_t)(k % (uint32_t)N), iy = (int32_t)((k / (uint32_t)N) % (uint32_t)N), iz = (int32_t)(k / (uint32_t)(N * N));
    long long b[kSeedMoments];   // the block's sums, untranslated
#pragma unroll
    for (int m = 0; m < kSeedMoments; ++m) b[m] = 0;
    // the 27 cells of the block, the centre among them; an index outside [0, N) on any axis is skipped, never wrapped: 27 trips
    for (int32_t d = 0; d < 27; ++d) {
      const int32_t jx = ix + d % 3 - 1, jy = iy + (d / 3) % 3 - 1, jz = iz + d / 9 - 1;
      if (jx < 0 || jx >= N || jy < 0 || jy >= N || jz < 0 || jz >= N) continue;
      const uint32_t slot = d == 13 ? 0u : find_slot(tab, fr, (uint32_t)(jx + N * (jy + N * jz)));
      if (slot == kSeedEmpty) continue;
      const uint32_t j = d == 13 ? i : c.tab_ord[fr.tab_beg + slot];
      const long long* src = c.mom + (fr.pt_beg + j) * kSeedMoments;
#pragma unroll
      for (int m = 0; m < kSeedMoments; ++m) b[m] += src[m];
    }
    long long own[kSeedMoments];
    {
      const long long* src = c.mom + (fr.pt_beg + i) * kSeedMoments;
#pragma unroll
      for (int m = 0; m < kSeedMoments; ++m) own[m] = src[m];
    }
    // exact translation to the centre cell's origin; then n_b sum q' q'^T - sum q' sum q'^T stays in int64: the host admits a
    // frame only while n 2 cq < 2^31, and |q'| <= 2 cq
    const long long o[3] = {(long long)c.g.cq * (ix - c.g.off), (long long)c.g.cq * (iy - c.g.off), (long long)c.g.cq * (iz - c.g.off)};
    long long tb[kSeedMoments], to[kSeedMoments];
    translate(b, o, tb);
    translate(own, o, to);
    const long long nb_i = tb[0];
    const double cxx = (double)(nb_i * tb[4] - tb[1] * tb[1]), cxy = (double)(nb_i * tb[5] - tb[1] * tb[2]), cxz = (double)(nb_i * tb[6] - tb[1] * tb[3]);
    const double cyy = (double)(nb_i * tb[7] - tb[2] * tb[2]), cyz = (double)(nb_i * tb[8] - tb[2] * tb[3]), czz = (double)(nb_i * tb[9] - tb[3] * tb[3]);
    const double cov[9] = {cxx, cxy, cxz, cxy, cyy, cyz, cxz, cyz, czz};
    double w[3], v[3][3];
    eig3_sym(cov, w, v);
    const double nb = (double)nb_i, nb2 = nb * nb;
    const bool flat = w[0] <= nb2 * c.flat_q2;
    const bool surface = 12.0 * w[1] >= nb2 * c.spread_q2;
    // A = the second moment of the cell's OWN points about the block's centroid m = sum_b q' / n_b
    const double no = (double)to[0];
    const double mc[3] = {(double)tb[1] / nb, (double)tb[2] / nb, (double)tb[3] / nb};
    const double sd[3] = {(double)to[1], (double)to[2], (double)to[3]};
    const double ssd[3][3] = {{(double)to[4], (double)to[5], (double)to[6]}, {(double)to[5], (double)to[7], (double)to[8]}, {(double)to[6], (double)to[8], (double)to[9]}};
    double r[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double A[3];
#pragma unroll
      for (int e = 0; e < 3; ++e) A[e] = ((ssd[a][e] - mc[a] * sd[e]) - mc[e] * sd[a]) + (no * mc[a]) * mc[e];
      r[a] = (A[0] * v[0][0] + A[1] * v[0][1]) + A[2] * v[0][2];
    }
    const double quad = (v[0][0] * r[0] + v[0][1] * r[1]) + v[0][2] * r[2];
    const bool own_in = quad <= no * c.own_q2;
    c.core[fr.pt_beg + i] = (flat && surface && own_in) ? 1 : 0;
  }
}

// root of x, with path halving.  key[parent[c]] < key[c] for every non-root c, so the keys along the chain strictly decrease:
// at most (cells of the frame) steps.  Halving only ever replaces a non-root's parent by that parent's parent -- an ancestor with
// a smaller key still -- and never touches a root, so it cannot undo or fake a link
__device__ __forceinline__ uint32_t find_root(uint32_t* parent, uint32_t x) {
  // strictly decreasing keys: at most (cells of the frame) steps
  for (;;) {
    const uint32_t p = ld(&parent[x]);
    if (p == x) return x;
    const uint32_t gp = ld(&parent[p]);
    if (gp != p) __atomic_store_n(&parent[x], gp, __ATOMIC_RELAXED);
    x = gp;
  }
}

// the same without writing (launches behind the union: the forest no longer changes)
__device__ __forceinline__ uint32_t read_root(const uint32_t* parent, uint32_t x) {
  // strictly decreasing keys: at most (cells of the frame) steps
  for (;;) {
    const uint32_t p = parent[x];
    if (p == x) return x;
    x = p;
  }
}

__device__ __forceinline__ void unite(uint32_t* parent, const uint32_t* key, uint32_t a, uint32_t b) {
  // Every failed compare-and-swap means another lane hung the root we held under a smaller key: the component's root key strictly
  // decreased.  At most (cells of the frame) retries; nobody is waited for
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    if (key[a] > key[b]) {   // a: the smaller key, stays root
      const uint32_t t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(&parent[b], b, a) == b) return;
  }
}

// kCore (K15p): only core cells are united, with core cells
template <bool kCore>
__global__ __launch_bounds__(kSeedThreads) void k15_union(SeedCtx c) {
  const uint32_t f = blockIdx.y;
  const SeedFrame fr = c.fr[f];
  const uint32_t n_cells = c.counters[2 * f];
  const uint32_t* tab = c.tab_key + fr.tab_beg;
  const uint32_t* key = c.cell_key + fr.pt_beg;
  uint32_t* parent = c.parent + fr.pt_beg;
  const int32_t N = c.g.N;
  const uint32_t stride = gridDim.x * kSeedThreads;
  // ceil(n_cells / stride) trips
  for (uint32_t i = blockIdx.x * kSeedThreads + threadIdx.x; i < n_cells; i += stride) {
    if (kCore && !c.core[fr.pt_beg + i]) continue;
    const uint32_t k = key[i];
    const int32_t ix = (int32_t)(k % (uint32_t)N), iy = (int32_t)((k / (uint32_t)N) % (uint32_t)N), iz = (int32_t)(k / (uint32_t)(N * N));
    // the 13 neighbours with a larger key: (dz, dy, dx) > (0, 0, 0) in that order = offsets 14 .. 26 of the 3 x 3 x 3 block: 13 trips
    for (int32_t d = 14; d < 27; ++d) {
      const int32_t dx = d % 3 - 1, dy = (d / 3) % 3 - 1, dz = d / 9 - 1;
      const int32_t jx = ix + dx, jy = iy + dy, jz = iz + dz;
      if (jx < 0 || jx >= N || jy < 0 || jy >= N || jz < 0 || jz >= N) continue;
      const uint32_t slot = find_slot(tab, fr, (uint32_t)(jx + N * (jy + N * jz)));
      if (slot == kSeedEmpty) continue;
      const uint32_t j = c.tab_ord[fr.tab_beg + slot];
      if (kCore && !c.core[fr.pt_beg + j]) continue;
      unite(parent, key, i, j);
    }
  }
}

// (K15p: a cell that is not core was never united, so it is its own root and adds nothing: only core non-roots add to their root)
__global__ __launch_bounds__(kSeedThreads) void k15_reduce(SeedCtx c) {
  const uint32_t f = blockIdx.y;
  const SeedFrame fr = c.fr[f];
  const uint32_t n_cells = c.counters[2 * f];
  const uint32_t* parent = c.parent + fr.pt_beg;
  const uint32_t stride = gridDim.x * kSeedThreads;
  const int lane = threadIdx.x & 63;
  // ceil(n_cells / stride) trips, the same for every lane of the workgroup
  for (uint32_t base = blockIdx.x * kSeedThreads; base < n_cells; base += stride) {
    const uint32_t i = base + threadIdx.x;
    uint32_t r = kNoCell;   // the root this lane's cell adds to; kNoCell: no cell, or a root (nothing to add)
    if (i < n_cells) {
      r = read_root(parent, i);
      if (r == i) r = kNoCell;
    }
    long long v[kSeedMoments];
    const long long* src = c.mom + (fr.pt_beg + (r != kNoCell ? i : 0u)) * kSeedMoments;   // a non-root's moments: nobody adds to them in this launch
#pragma unroll
    for (int m = 0; m < kSeedMoments; ++m) v[m] = r != kNoCell ? src[m] : 0;
    // Most of a wavefront's cells hang under one or two roots (the ground, a wall): the lanes of one root are summed across the
    // wavefront and ONE lane adds the total, instead of thousands of cells queueing on the root's ten words.
    // At most 64 trips: every trip retires all lanes of one root
    for (unsigned long long todo = __ballot(r != kNoCell); todo != 0ull; todo = __ballot(r != kNoCell)) {
      const uint32_t root = __shfl(r, __ffsll((long long)todo) - 1, 64);
      const bool mine = r == root;
#pragma unroll
      for (int m = 0; m < kSeedMoments; ++m) {
        long long t = mine ? v[m] : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);   // the total arrives in lane 0
        if (lane == 0) add64(c.mom + (fr.pt_beg + root) * kSeedMoments + m, t);
      }
      if (mine) r = kNoCell;
    }
  }
}

// kCore (K15p): only core roots claim a record
template <bool kCore>
__global__ __launch_bounds__(kSeedThreads) void k15_pack(SeedCtx c) {
  const uint32_t f = blockIdx.y;
  const SeedFrame fr = c.fr[f];
  const uint32_t n_cells = c.counters[2 * f];
  const uint32_t stride = gridDim.x * kSeedThreads;
  // ceil(n_cells / stride) trips
  for (uint32_t i = blockIdx.x * kSeedThreads + threadIdx.x; i < n_cells; i += stride) {
    if (c.parent[fr.pt_beg + i] != i) continue;
    if (kCore && !c.core[fr.pt_beg + i]) continue;
    const long long* m = c.mom + (fr.pt_beg + i) * kSeedMoments;
    if (m[0] < (long long)c.cluster_min) continue;
    const uint32_t at = atomicAdd(&c.counters[2 * f + 1], 1u);   // the count goes on past max_components: the host reports ILCC_CAPACITY
    if (at >= c.max_components) continue;
    long long* rec = c.packed + ((uint64_t)f * c.max_components + at) * ILCC_SEED_RECORD_WORDS;
    rec[0] = (long long)c.cell_key[fr.pt_beg + i];
#pragma unroll
    for (int k = 0; k < kSeedMoments; ++k) rec[1 + k] = m[k];
  }
}

void launch_seed_components(const SeedCtx& c, uint32_t max_frame_points, hipStream_t s, const hipEvent_t* between) {
  // blocks per frame: one lane per point of the largest frame, at most 1024 blocks (a lane then takes several points)
  uint32_t bx = (max_frame_points + kSeedThreads - 1) / kSeedThreads;
  bx = bx < 1u ? 1u : (bx > 1024u ? 1024u : bx);
  const dim3 grid(bx, c.n_frames), block(kSeedThreads);
  const uint64_t clear_blocks = (c.slots_total + kSeedThreads - 1) / kSeedThreads;
  int k = 0;
  auto mark = [&]() {
    if (between) (void)hipEventRecord(between[k++], s);
  };
  mark();
  hipLaunchKernelGGL(k15_clear, dim3((uint32_t)(clear_blocks > 65536u ? 65536u : clear_blocks)), block, 0, s, c);
  mark();
  hipLaunchKernelGGL(k15_insert, grid, block, 0, s, c);
  mark();
  hipLaunchKernelGGL(k15_moments, grid, block, 0, s, c);
  mark();
  if (c.core) {
    hipLaunchKernelGGL(k15_classify, grid, block, 0, s, c);
    mark();
    hipLaunchKernelGGL(k15_union<true>, grid, block, 0, s, c);
  } else {
    hipLaunchKernelGGL(k15_union<false>, grid, block, 0, s, c);
  }
  mark();
  hipLaunchKernelGGL(k15_reduce, grid, block, 0, s, c);
  mark();
  if (c.core)
    hipLaunchKernelGGL(k15_pack<true>, grid, block, 0, s, c);
  else
    hipLaunchKernelGGL(k15_pack<false>, grid, block, 0, s, c);
  mark();
}

}  // namespace ilcc
