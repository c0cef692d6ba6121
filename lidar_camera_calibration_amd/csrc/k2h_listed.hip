// k2h_listed.hip -- the second tier of the online caller: the k2h_* chain of kernels, which runs the hashed-cell phases of
// k2_hashed.h over the listed frames with the whole chip, and its launcher launch_cluster_listed (called by ilcc_api.cpp).
//
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
#include "k2_hashed.h"
#include "k2_point_level.h"

namespace ilcc {

constexpr int kListChunk = 256;       // items per work item
constexpr int kListBlock = 1024;      // listed frames whose chunk prefix sums a workgroup keeps in LDS at a time
struct ListedFrame {   // per frame (indexed by frame, valid for listed frames)
  HashFrame g;
  uint32_t n_cells;
  uint32_t valid;      // 0: outside the hashed path's limits: k2h_finish clusters the frame with the point-level search
  uint32_t pad[6];
};
static_assert(sizeof(ListedFrame) == kListedFrameBytes, "the handle allocates kListedFrameBytes per frame");

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

// one thread per ROI point i of the listed frames inside the hashed path's limits: fn(the frame's views, f, i)
template <typename Fn>
__device__ __forceinline__ void for_each_listed_point(const Ctx& c, const ListedFrame* frames, uint32_t* s_pref, Fn fn) {
  for_each_listed_chunk(c, s_pref, [&](uint32_t f) { return frames[f].valid ? (uint32_t)c.res[f].n_roi : 0u; }, [&](uint32_t f, uint32_t first) {
    const HashViews v = hash_views(c, f);
    const uint32_t i = first + threadIdx.x;
    if (i < v.M) fn(v, f, i);
  });
}

// one thread per occupied cell A of the listed frames (a frame outside the limits has none): fn(f, A)
template <typename Fn>
__device__ __forceinline__ void for_each_listed_cell(const Ctx& c, const ListedFrame* frames, uint32_t* s_pref, Fn fn) {
  for_each_listed_chunk(c, s_pref, [&](uint32_t f) { return frames[f].n_cells; }, [&](uint32_t f, uint32_t first) {
    const uint32_t A = first + threadIdx.x;
    if (A >= frames[f].n_cells) return;
    fn(f, A);
  });
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
  for_each_listed_point(c, frames, s_pref, [&](const HashViews& v, uint32_t f, uint32_t i) { hash_insert<AgentScope>(v, frames[f].g, i); });
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
  for_each_listed_point(c, frames, s_pref, [&](const HashViews& v, uint32_t, uint32_t i) { hash_cell<AgentScope>(v, i); });
}

__global__ __launch_bounds__(1024) void k2h_starts(Ctx c, const ListedFrame* frames) {
  __shared__ uint32_t sc[32];
  uint32_t f;
  if (!listed_frame(c, f) || !frames[f].valid) return;
  hash_starts(hash_views(c, f), frames[f].n_cells, sc);
}

__global__ __launch_bounds__(kListChunk) void k2h_place(Ctx c, const ListedFrame* frames) {
  __shared__ uint32_t s_pref[kListBlock + 1];
  for_each_listed_point(c, frames, s_pref, [&](const HashViews& v, uint32_t, uint32_t i) { hash_place<AgentScope>(v, i); });
}

__global__ __launch_bounds__(kListChunk) void k2h_edges(Ctx c, const ListedFrame* frames) {
  __shared__ uint32_t s_pref[kListBlock + 1];
  const float tol2 = (float)(c.p.cluster_tol * c.p.cluster_tol);
  for_each_listed_cell(c, frames, s_pref, [&](uint32_t f, uint32_t A) {
    AgentScope::Clock clk;
    hash_edges<AgentScope>(hash_views(c, f), frames[f].g, A, tol2, clk);
  });
}

__global__ __launch_bounds__(kListChunk) void k2h_roots(Ctx c, const ListedFrame* frames) {
  __shared__ uint32_t s_pref[kListBlock + 1];
  for_each_listed_cell(c, frames, s_pref, [&](uint32_t f, uint32_t A) {
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

// the flagged frames, listed (one thread per frame: a few dozen frames at most matter)
__global__ __launch_bounds__(256) void k2h_list(Ctx c) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < c.n_frames && c.frame_flags[f] != 0u && c.res[f].status == ILCC_OK) c.list[atomicAdd(c.list_count, 1u)] = f;
}

// the frames the online caller's first tier could not vouch for: the chain over the listed frames
void launch_cluster_listed(const Ctx& c, hipStream_t s) {
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
}

}  // namespace ilcc
