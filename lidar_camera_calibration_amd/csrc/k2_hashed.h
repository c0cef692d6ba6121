// k2_hashed.h -- components on cells with the cells in a HASH TABLE in global memory (round 5): the phases hash_setup ...
// hash_tail, their types and the two memory-scope policies they are instantiated with.  Included by k2_fallback.hip
// (hashed_cluster_frame: one workgroup per frame, WgScope) and by k2h_listed.hip (the k2h_* chain, AgentScope).
//
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
//   the k2h_* chain (AgentScope): several workgroups share a frame, so atomics and the loads that race them are agent-scope.
// Scratch per frame (all dead at K2 time, rewritten by K3 / K4 / K5 / K5w / K7b afterwards): table keys = the frame's slice of
// uf_hash_head; base ids = board; masks = pca (low words) + optim (high words); per point / per cell words = uf_hash_next
// (cell of a point), uf_count (count, later component size), uf_parent (cell union-find), yz (smallest index | block-and-bit,
// later the root), walk_yz (sorted start).  Same cells, same pair arithmetic, same union rule, labels = smallest member index:
// the partition, the choice and the index-ordered output are those of the other paths (tests: the online caller, the wide sparse
// ROI and the large ROIs against the oracle's BFS).
#pragma once

#include "k2_common.h"

namespace ilcc {

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
// The counters of the edge search and of the one-workgroup union-find, as a policy: nothing here.  A -DILCC_K2_TIMING build of
// k2_fallback.hip gives the one-workgroup path a clock that counts (EdgeClock there, beside the device globals it adds to).
struct NoClock {
  __device__ void lap(int) {}
  __device__ void pair() {}
  __device__ void hit() {}
  __device__ void flush() {}
  static __device__ void find() {}
  static __device__ void hop() {}
};
// union-find on global parents owned by ONE workgroup: plain loads (a stale parent is still an ancestor: parents only move to
// smaller indices), hooks by workgroup-scope compare-and-swap; a failed hook continues from the parent the CAS returned
template <class Clock>
__device__ __forceinline__ uint32_t wg_find(uint32_t* parent, uint32_t x) {
  Clock::find();
  for (;;) {
    Clock::hop();
    const uint32_t p = parent[x];
    if (p == x) return x;
    const uint32_t gp = parent[p];
    if (gp != p) parent[x] = gp;   // path halving (a non-root's word: hooks only ever touch roots)
    x = p;
  }
}
template <class Clock>
__device__ __forceinline__ void wg_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = wg_find<Clock>(parent, a);
    b = wg_find<Clock>(parent, b);
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
template <class ClockT>
struct WgScope {   // hashed_cluster_frame: one workgroup owns the frame
  static constexpr int kScope = __HIP_MEMORY_SCOPE_WORKGROUP;
  using Clock = ClockT;
  static __device__ __forceinline__ uint32_t load(const uint32_t* p) { return *p; }
  static __device__ __forceinline__ uint32_t cas(uint32_t* p, uint32_t expect, uint32_t desired) { return wg_cas(p, expect, desired); }
  static __device__ __forceinline__ uint32_t find(uint32_t* parent, uint32_t x) { return wg_find<Clock>(parent, x); }
  static __device__ __forceinline__ void unite(uint32_t* parent, uint32_t a, uint32_t b) { wg_unite<Clock>(parent, a, b); }
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
// until the first hit (ref_dist2) and the cells united (hooks to the smaller id)
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
          for (uint32_t k = 0; k < 4u; ++k) hit |= ref_dist2(q[k].x - pa.x, q[k].y - pa.y, q[k].z - pa.z) < tol2;
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

}  // namespace ilcc
