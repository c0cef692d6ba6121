// k2_point_level.h -- the point-level spatial hash of rounds 1-3 by one workgroup: the last resort for a frame beyond the limits
// of both cell paths (k2_common.h).  Called by k2_fallback_cluster (k2_fallback.hip) and by k2h_finish (k2h_listed.hip).
#pragma once

#include "k2_common.h"

namespace ilcc {

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
            if (ref_dist2(q.x - pi.x, q.y - pi.y, q.z - pi.z) < tol2) {
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

// Components are the points that are roots (the smallest member index), their sizes counted on the root.
__device__ inline void point_level_cluster_frame(const Ctx& c, uint32_t f, uint32_t* sc) {
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

}  // namespace ilcc
