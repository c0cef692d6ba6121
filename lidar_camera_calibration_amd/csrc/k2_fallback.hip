// k2_fallback.hip -- K2's fallback launch, k2_fallback_cluster: the frames k2_seeded_cluster (k2_cluster.hip) listed because its
// LDS cell grid could not hold them -- a bounding grid above the bitmap, more occupied cells than the capacity -- each by one
// workgroup on hashed cells (hashed_cluster_frame, the phases of k2_hashed.h) and on points beyond that path's limits
// (k2_point_level.h).  Few frames of real recordings come here and none of the bench's; inlined behind the LDS-grid path this
// code doubled the registers of every K2 wavefront.  The launcher: launch_cluster_fallback, called by launch_cluster.
#include "k2_hashed.h"
#include "k2_point_level.h"

namespace ilcc {

// ------------------------------------------------------------------ hashed cells by the frame's own workgroup
// -DILCC_K2_TIMING: counters of the one-workgroup path's edge search (union-find hops, cell pairs tested, thread-cycles per part).
// Device globals, so defined in this file only; the k2h_* chain runs with NoClock.
#ifdef ILCC_K2_TIMING
__device__ unsigned long long g_k2_hops, g_k2_finds, g_k2_pairs, g_k2_hits, g_k2_t[6];
struct EdgeClock {
  unsigned long long t[6] = {0, 0, 0, 0, 0, 0}, last = __builtin_readcyclecounter();
  __device__ void lap(int k) {
    const unsigned long long now = __builtin_readcyclecounter();
    t[k] += now - last;
    last = now;
  }
  __device__ void pair() { atomicAdd(&g_k2_pairs, 1ull); }
  __device__ void hit() { atomicAdd(&g_k2_hits, 1ull); }
  __device__ void flush() {
    for (int k = 0; k < 6; ++k) atomicAdd(&g_k2_t[k], t[k]);
  }
  static __device__ void find() { atomicAdd(&g_k2_finds, 1ull); }
  static __device__ void hop() { atomicAdd(&g_k2_hops, 1ull); }
};
#else
using EdgeClock = NoClock;
#endif
using FrameScope = WgScope<EdgeClock>;

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
  for (uint32_t i = tid; i < M; i += kT) hash_insert<FrameScope>(v, g, i);
  wg_phase();
  HC_MARK(3);
  const uint32_t C = hash_blocks(v, g, sc);
  wg_phase();
  HC_MARK(4);
  for (uint32_t i = tid; i < M; i += kT) hash_cell<FrameScope>(v, i);
  wg_phase();
  HC_MARK(5);
  hash_starts(v, C, sc);
  wg_phase();
  for (uint32_t i = tid; i < M; i += kT) hash_place<FrameScope>(v, i);
  wg_phase();
  HC_MARK(6);
  {
    const float tol2 = (float)(c.p.cluster_tol * c.p.cluster_tol);
    FrameScope::Clock clk;
    for (uint32_t A = tid; A < C; A += kT) hash_edges<FrameScope>(v, g, A, tol2, clk);
    clk.flush();
  }
  wg_phase();
  HC_MARK(7);
  for (uint32_t t0 = 0; t0 < C; t0 += kT) {
    const uint32_t A = t0 + tid;
    uint32_t root = 0;
    if (A < C) root = FrameScope::find(v.cpar, A);
    wg_phase();   // (path halving rewrites parents: finish every find of the tile before the roots are stored)
    if (A < C) hash_root<FrameScope>(v, A, root);
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

// ------------------------------------------------------------------ the kernels and their launcher
// one listed frame by this workgroup
__device__ __forceinline__ void fallback_frame(const Ctx& c, uint32_t f, uint32_t* sc) {
  // the same components on cells with the cells in a hash table (global memory) ...
  if (hashed_cluster_frame(c, f, sc)) return;
  // ... and beyond that path's limits (> 65 536 ROI points in one frame, a bounding grid of > 2^32 blocks): point-level search
  __syncthreads();
  point_level_cluster_frame(c, f, sc);
}

// A fixed grid: workgroup b runs items b, b + gridDim.x, ... of Ctx::fallback_list.  The count is final (k2_seeded_cluster has
// finished: same stream) and read once; it is usually 0, and every workgroup returns on that load.  256 threads: inside the
// loop the body takes 137 VGPRs, and under a 1024-thread bound (128 VGPRs) the compiler spills to scratch memory, which
// every dispatch then has to be given, an empty one included.
__global__ __launch_bounds__(256) void k2_fallback_cluster(Ctx c) {
  __shared__ uint32_t sc[160];
  const uint32_t count = (uint32_t)c.grid_iters[kFallbackWord];
  for (uint32_t item = blockIdx.x; item < count; item += gridDim.x) {
    if (item != blockIdx.x) __syncthreads();   // (sc is reused: the frame before is done with it)
    fallback_frame(c, c.fallback_list[item], sc);
  }
}
// ... and behind a 1024-thread launch, a batch of at most kSmallBatchFrames frames: a workgroup per frame of the batch covers
// any list, so workgroup b has item b alone and no loop (89 VGPRs)
__global__ __launch_bounds__(1024) void k2_fallback_cluster_wide(Ctx c) {
  __shared__ uint32_t sc[160];
  if (blockIdx.x < (uint32_t)c.grid_iters[kFallbackWord]) fallback_frame(c, c.fallback_list[blockIdx.x], sc);
}

// Behind k2_seeded_cluster on its stream, at its thread count (a launch wider than 256 threads whose batch exceeds the grid,
// which no batch size of this build gives, would take the looping kernel at 256): min(frames, kFallbackGrid) workgroups -- a batch cannot list more
// frames than it has.  kFallbackGrid = 1024 is a frame per workgroup slot of the chip at 256 threads, as k2_seeded_cluster ran
// these frames.  Measured ("K2's fallback in a launch of its own"): the empty launch costs 4.2 us alone at
// 256 and at 1024 workgroups alike, a 1984-frame batch whose every frame is listed 0.59 ms against 0.55 ms inside k2_seeded_cluster.
void launch_cluster_fallback(const Ctx& c, hipStream_t s, uint32_t threads) {
  const dim3 grid(std::min(c.n_frames, kFallbackGrid));
  if (threads > 256u && c.n_frames <= kFallbackGrid)
    hipLaunchKernelGGL(k2_fallback_cluster_wide, grid, dim3(threads), 0, s, c);
  else
    hipLaunchKernelGGL(k2_fallback_cluster, grid, dim3(std::min(threads, 256u)), 0, s, c);
}

}  // namespace ilcc
