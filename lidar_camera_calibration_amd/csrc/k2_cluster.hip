// k2_cluster.hip -- K2's per-frame launch, k2_seeded_cluster: one workgroup per frame on the LDS cell grid (fine_cluster_frame);
// a frame the grid cannot hold is listed for k2_fallback_cluster (k2_fallback.hip: hashed cells, and points beyond that), which
// launch_cluster launches right behind it.  Its LDS size, device limits and launcher (launch_cluster).  The cell argument and
// which frame takes which path: k2_common.h.  The online caller's second tier is k2h_listed.hip.
#include "k2_common.h"

namespace ilcc {

// ------------------------------------------------------------------ components on cells (the ROI case)
constexpr int kFineBitsOnline = 128 * 1024;      // ... in the first tier of the online caller: a +-1.25 m window at tol 0.10 is <= 49^3 = 118 k cells padded
constexpr int kFineBits = 96 * 1024;             // cells of the padded bounding grid the bitmap holds (12 KiB); a 2 x 3 x 4 m ROI box at
                                                 // tol 0.12 is <= 34 x 48 x 63 = 102 k cells padded, the bounding box of real ROI clouds ~50 k
__host__ __device__ inline uint32_t fine_words(uint32_t bits) { return bits / 32u + 2u; }   // + 2: the 5-bit neighbour windows read one word past their own
// the 13 forward (dy, dz) rows of the 5 x 5 x 5 neighbourhood, nearest first: row 0 is the cell's own row (dx = +1, +2), every
// other row a window of five cells dx = -2..2.  A pair of cells is met once, from the one with the smaller (z, y, x).
__device__ const signed char kRowDy[13] = {0, 1, 0, 1, -1, 2, 0, 2, -2, 1, -1, 2, -2};
__device__ const signed char kRowDz[13] = {0, 0, 1, 1, 1, 0, 2, 1, 1, 2, 2, 2, 2};

struct FineGrid {
  float3 lo;
  float inv;
  int nx, ny, nz;
  uint32_t n_w32, n_w64;   // words of the bitmap the grid's cells take (32-bit: + 2 as fine_words; 64-bit)
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

// ---- the steps of the LDS-grid path, in the order fine_cluster_frame runs them.  Every thread of the frame's workgroup calls
// each; none has a barrier of its own beyond those of the block-wide helper it names: fine_cluster_frame places them.

// setup: bounding box (block_bbox; sc: 112 floats, free on return), grid dimensions.  False (uniformly): the extent is too large
// or the padded bounding grid has more cells than the bitmap holds.  Touches no other LDS.
__device__ __forceinline__ bool fine_setup(const Ctx& c, const float4* __restrict__ P, uint32_t M, uint32_t* sc, FineGrid& g) {
  float3 lo, hi;
  block_bbox(P, M, reinterpret_cast<float*>(sc), lo, hi);
  g.lo = lo;
  g.inv = 1.0f / ((float)c.p.cluster_tol * kFineCellOverTol);
  const float ex = (hi.x - lo.x) * g.inv, ey = (hi.y - lo.y) * g.inv, ez = (hi.z - lo.z) * g.inv;
  if (!(ex < 8192.f && ey < 8192.f && ez < 8192.f)) return false;   // (also catches a NaN extent)
  g.nx = (int)floorf(ex) + 5;
  g.ny = (int)floorf(ey) + 5;
  g.nz = (int)floorf(ez) + 5;
  const unsigned long long cells = (unsigned long long)g.nx * (unsigned long long)g.ny * (unsigned long long)g.nz;
  if (cells > (unsigned long long)c.cluster_bits) return false;
  g.n_w32 = ((uint32_t)cells + 31u) / 32u + 2u;
  g.n_w64 = ((uint32_t)cells + 63u) / 64u;
  return true;
}

// occupancy bitmap: bm all zero (whole 64-bit words) ...
__device__ __forceinline__ void fine_bitmap_clear(const FineLds& L, const FineGrid& g) {
  for (uint32_t k = threadIdx.x; k < ((g.n_w32 + 1u) & ~1u); k += blockDim.x) L.bm[k] = 0u;
}
// ... then a bit per occupied cell.  bm is final from the barrier behind this.
__device__ __forceinline__ void fine_bitmap_mark(const FineLds& L, const FineGrid& g, const float4* __restrict__ P, uint32_t M) {
  for (uint32_t i = threadIdx.x; i < M; i += blockDim.x) {
    const uint32_t key = fine_key(g, P[i]);
    atomicOr(&L.bm[key >> 5], 1u << (key & 31u));
  }
}
// rank directory: reads bm; returns the number of occupied cells C to every thread (block_excl_scan, sc: 17 words) and records
// its maximum.  Writes pre (final from the next barrier) unless C is above the cell arrays' capacity: the caller refuses the frame.
__device__ __forceinline__ uint32_t fine_rank_directory(const Ctx& c, const FineLds& L, const FineGrid& g) {
  unsigned long long* stats = c.grid_iters + 3 * kIterSlots;   // [0] most occupied cells a frame needed
  const uint32_t tid = threadIdx.x, kT = blockDim.x;
  uint32_t C = 0;
  const unsigned long long* bm64 = reinterpret_cast<const unsigned long long*>(L.bm);
  const uint32_t per = (g.n_w64 + kT - 1u) / kT, w0 = tid * per, w1 = min(g.n_w64, w0 + per);
  uint32_t sum = 0;
  for (uint32_t w = w0; w < w1; ++w) sum += (uint32_t)__popcll(bm64[w]);
  uint32_t run = block_excl_scan(sum, L.sc, C);
  if (C <= c.cluster_cells_cap)
    for (uint32_t w = w0; w < w1; ++w) {
      L.pre[w] = (uint16_t)run;
      run += (uint32_t)__popcll(bm64[w]);
    }
  if (tid == 0) atomicMax(&stats[0], (unsigned long long)C);
  return C;
}

// cells: ccnt = 0 and cmin = none for the C cells ...
__device__ __forceinline__ void fine_cells_reset(const FineLds& L, uint32_t C) {
  for (uint32_t k = threadIdx.x; k < C; k += blockDim.x) {
    L.ccnt[k] = 0u;
    L.cmin[k] = 0xFFFFFFFFu;
  }
}
// ... then, reading bm and pre: ccnt = points, cmin = smallest member index, ckey = key of every occupied cell
__device__ __forceinline__ void fine_cells(const FineLds& L, const FineGrid& g, const float4* __restrict__ P, uint32_t M) {
  for (uint32_t i = threadIdx.x; i < M; i += blockDim.x) {
    const uint32_t key = fine_key(g, P[i]);
    const uint32_t cid = fine_rank(L.bm, L.pre, key);
    atomicAdd(&L.ccnt[cid], 1u);
    atomicMin(&L.cmin[cid], i);
    L.ckey[cid] = key;   // (every point of the cell writes the same word)
  }
}

// starts: cstart[k] = first sorted position of cell k, the exclusive scan of ccnt (block_excl_scan, sc: 17 words); cstart[C] = M
__device__ __forceinline__ void fine_starts(const FineLds& L, uint32_t C, uint32_t M) {
  const uint32_t tid = threadIdx.x, kT = blockDim.x;
  const uint32_t per = (C + kT - 1u) / kT, k0 = tid * per, k1 = min(C, k0 + per);
  uint32_t sum = 0, tot;
  for (uint32_t k = k0; k < k1; ++k) sum += L.ccnt[k];
  uint32_t run = block_excl_scan(sum, L.sc, tot);
  for (uint32_t k = k0; k < k1; ++k) {
    L.cstart[k] = run;
    run += L.ccnt[k];
  }
  if (tid == 0) L.cstart[C] = M;
}

// placement: the points sorted by cell into their home, sx / sy / sz or gpts (the order inside a cell is the race of the atomics:
// nothing below depends on it), counting ccnt down: it LEAVES ccnt ALL ZERO, which the component sizes rely on.  Every cell
// becomes its own root in cpar.
template <bool PTS_LDS>
__device__ __forceinline__ void fine_place(const FineLds& L, const FineGrid& g, const float4* __restrict__ P, uint32_t M, float4* gpts,
                                           uint32_t C) {
  const uint32_t tid = threadIdx.x, kT = blockDim.x;
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
}

// the pair test of two cells: does some point of A = [a0, a1) lie within the tolerance of some point of B = [b0, b1) (sorted
// positions; ref_dist2 against tol2)?
// A's point once per ia, B's points kGroup at a time: the group's loads are unconditional (an index past the cell's
// end reads its last point again: harmless) and independent, one round trip per group instead of one per test -- at L2
// latency (the points in `cluster`) the serial walk was the frame's chain.  Same tests, same arithmetic; which pair hits
// first does not matter, only whether one does
template <bool PTS_LDS>
__device__ __forceinline__ bool fine_cells_touch(const FineLds& L, const float4* gpts, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1,
                                                 float tol2) {
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
      for (uint32_t k = 0; k < kGroup; ++k) nearest = fminf(nearest, ref_dist2(q[k].x - p.x, q[k].y - p.y, q[k].z - p.z));
      hit = nearest < tol2;
    }
  }
  return hit;
}

// edges between cells: reads bm, pre, ckey, cstart and the sorted points, unites in cpar.  (row, cell) items, rows outermost: by
// the time the far rows come up most cells of a surface already share a root and a pair costs two finds.
template <bool PTS_LDS>
__device__ __forceinline__ void fine_edges(const FineLds& L, const FineGrid& g, const float4* gpts, uint32_t C, float tol2) {
  for (int row = 0; row < 13; ++row) {
    const int delta = (int)kRowDy[row] * g.nx + (int)kRowDz[row] * g.nx * g.ny;
    for (uint32_t A = threadIdx.x; A < C; A += blockDim.x) {
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
        if (fine_cells_touch<PTS_LDS>(L, gpts, a0, a1, L.cstart[B], L.cstart[B + 1], tol2)) uf_unite(L.cpar, ra, rb);
      }
    }
  }
}

// roots, a tile of one cell per thread: fine_cluster_frame finds the root of cell k (path halving rewrites parents), and behind a
// barrier stores it here.  ckey, free since the edges, IS REUSED for the component's smallest member index: none yet.
__device__ __forceinline__ void fine_store_root(const FineLds& L, uint32_t k, uint32_t root) {
  L.cpar[k] = root;
  L.ckey[k] = 0xFFFFFFFFu;
}
// component sizes: on every root, ccnt (all zero since the placement) = points of its cells, ckey = smallest member index of them
__device__ __forceinline__ void fine_components(const FineLds& L, uint32_t C) {
  for (uint32_t k = threadIdx.x; k < C; k += blockDim.x) {
    const uint32_t root = L.cpar[k];
    atomicAdd(&L.ccnt[root], L.cstart[k + 1] - L.cstart[k]);
    atomicMin(&L.ckey[root], L.cmin[k]);
  }
}

// The steps by the frame's workgroup, with the barriers between them.  Returns false (uniformly, and before any word of the
// frame's result is written) when the frame does not fit the grid / the cell capacity: the caller hands the frame to the fallback launch.
// (The tail stays written out here: as a step of its own it cost the kernel 86 scalar instructions and 16 SGPR spills.)
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

  FineGrid g;
  if (!fine_setup(c, P, M, sc, g)) return false;
  fine_bitmap_clear(L, g);
  __syncthreads();
  fine_bitmap_mark(L, g, P, M);
  __syncthreads();
  const uint32_t C = fine_rank_directory(c, L, g);
  if (C > c.cluster_cells_cap) return false;   // more occupied cells than the handle's LDS arrays hold: it grows them for the next batch
  __syncthreads();
  fine_cells_reset(L, C);
  __syncthreads();
  fine_cells(L, g, P, M);
  __syncthreads();
  fine_starts(L, C, M);
  __syncthreads();
  fine_place<PTS_LDS>(L, g, P, M, gpts, C);
  if (!PTS_LDS) __threadfence_block();
  __syncthreads();
  fine_edges<PTS_LDS>(L, g, gpts, C, tol2);
  __syncthreads();
  for (uint32_t base = 0; base < C; base += kT) {
    const uint32_t k = base + tid;
    uint32_t root = 0;
    if (k < C) root = uf_find(L.cpar, k);
    __syncthreads();   // (path halving rewrites parents: finish every find of the tile before the roots are stored)
    if (k < C) fine_store_root(L, k, root);
    __syncthreads();
  }
  fine_components(L, C);
  __syncthreads();

  // ---- the tail: exact 1-NN of the click, the choice (components: root cells, size in ccnt, smallest index in ckey; a
  // point's: its cell's root, through bm, pre and cpar)
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
  // stable compaction of the chosen component (index order), over the L2 home of the sorted points
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

// ------------------------------------------------------------------ the kernel, its LDS and its launcher
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
  // The LDS cell grid cannot hold this frame: k2_fallback_cluster, launched behind this kernel, clusters it on hashed cells or on
  // points.  fine_cluster_frame returned false before it wrote any word of the frame's result (record, `cluster`), so the
  // frame reaches that launch as K1 left it.  The fallback's code is kept out of this kernel for the registers it costs every
  // wavefront here: 113 VGPRs with it inlined, 59 without.
  if (threadIdx.x == 0) c.fallback_list[atomicAdd(c.grid_iters + kFallbackWord, 1ull)] = f;
}

// up to a CU's whole LDS as dynamic LDS (> the 64 KiB default cap).  Called by ilcc_create for the handle's device: the attribute
// is kept per (function, device).
hipError_t set_kernel_attributes_k2() {
  return hipFuncSetAttribute((const void*)k2_seeded_cluster, hipFuncAttributeMaxDynamicSharedMemorySize, kCuLdsBytes);
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
  const int threads = (c.n_frames <= (uint32_t)kSmallBatchFrames || c.wide) ? 1024 : kFrameThreads;   // (small batches: latency, not CU footprint, matters)
  const size_t with_copy = cluster_lds_bytes(c.cluster_lds_points, c.cluster_cells_cap, c.cluster_bits);
  if (home == kClusterHomeRule)
    home = (c.wide || c.n_frames <= cluster_resident_frames(lim, (uint32_t)threads, with_copy)) ? kClusterHomeLds : kClusterHomeL2;
  Ctx k = c;
  if (home == kClusterHomeL2) k.cluster_lds_points = 0u;   // no frame fits "the capacity": fine_cluster_frame<false> for all
  const size_t lds = cluster_lds_bytes(k.cluster_lds_points, k.cluster_cells_cap, k.cluster_bits);
  hipLaunchKernelGGL(k2_seeded_cluster, dim3(k.n_frames), dim3(threads), lds, s, k);
  // (the online caller's first tier flags the frames the grid cannot hold for its second tier instead of listing them)
  if (c.online_tier == 0u) launch_cluster_fallback(c, s, (uint32_t)threads);
  return ClusterLaunch{home, (uint32_t)lds, (uint32_t)threads};
}

}  // namespace ilcc
