// Result transport, called by the host API only: K9 packs a batch's records, k_store_to_host writes device words into pinned
// host memory.
#include <algorithm>

#include "ilcc_internal.h"

namespace ilcc {

// K9 pack_records: ilcc_result[] (device) -> fixed-size float records [n_frames, ILCC_RECORD_HEADER + 3 * n_corners]
// for the path's single collective (the gather of corner records): the records go from
// this GPU's HBM straight into RCCL, no host round trip.  Layout = sharding.pack_records.  tag = tag_base + frame
// and check = 24-bit xor-fold of the corner bits and the tag let the receiving rank verify WHOSE records arrived
// where and that their contents are intact (both are exact in a float).
__global__ __launch_bounds__(128) void k9_pack_records(const ilcc_result* __restrict__ res, uint32_t n_corners, uint32_t tag_base,
                                                       float* __restrict__ out) {
  __shared__ uint32_t s_x[2];
  const ilcc_result& r = res[blockIdx.x];
  const uint32_t width = (uint32_t)ILCC_RECORD_HEADER + 3u * n_corners;
  float* o = out + (uint64_t)blockIdx.x * width;
  const uint32_t have = (uint32_t)(r.n_corners < 0 ? 0 : r.n_corners);
  const uint32_t tag = (tag_base + blockIdx.x) & 0xFFFFFFu;
  uint32_t x = 0;
  for (uint32_t k = threadIdx.x; k < width; k += blockDim.x) {
    float v = 0.f;
    if (k >= (uint32_t)ILCC_RECORD_HEADER) {
      const uint32_t c = k - (uint32_t)ILCC_RECORD_HEADER;
      v = (c < 3u * have) ? r.corners[c] : 0.f;
      x ^= __float_as_uint(v) * (2u * c + 1u);   // position-dependent: swapped corners change the fold
    } else {
      switch (k) {
        case 0: v = (float)r.status; break;
        case 1: v = (float)r.n_corners; break;
        case 2: v = (float)r.phase; break;
        case 3: v = (float)r.grid_index; break;
        case 4: v = (float)r.iters_a; break;
        case 5: v = (float)r.iters_b; break;
        case 6: v = (float)r.cost_a; break;
        case 7: v = (float)r.cost_b; break;
        case 8: v = (float)r.sel_cost; break;
        case 9: v = (float)r.theta_t[0]; break;
        case 10: v = (float)r.theta_t[1]; break;
        case 11: v = (float)r.theta_t[2]; break;
        case 12: v = (float)r.n_plane; break;
        case 13: v = (float)r.n_black; break;
        case 14: v = (float)r.n_white; break;
        case 15: v = (float)r.basin_margin; break;
        case 16: v = (float)tag; break;
        case 18: v = (float)r.flags; break;
        case 19: v = (float)r.n_roi; break;
        default: v = 0.f;   // 17 (check) is written below
      }
    }
    if (k != 17u) o[k] = v;
  }
#pragma unroll
  for (int of = ILCC_WAVE / 2; of > 0; of >>= 1) x ^= __shfl_xor(x, of, ILCC_WAVE);
  if ((threadIdx.x & (ILCC_WAVE - 1)) == 0) s_x[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = s_x[0] ^ s_x[1] ^ (tag * 0x9E3779B1u);
    t = (t ^ (t >> 24)) & 0xFFFFFFu;
    o[17] = (float)t;
  }
}

// Device -> pinned HOST memory by a kernel's own stores (the staging buffers are hipHostMalloc'ed: mapped, fine-grained).  Round 6:
// a batch's result copies used to be hipMemcpyAsync(D2H) commands queued behind its kernels at submit time; the SDMA engine that
// also carries the NEXT batches' 472 MB input copies then sat on each of them until that batch's kernels had finished
// (tools/dev_h2d_probe.py: the H2D-inclusive pipeline moved 52.0 GB/s with kernels running against 56.3 GB/s with the kernels
// returning early) -- with the records written by the GPU itself the SDMA queue holds input copies only.
__global__ __launch_bounds__(256) void k_store_to_host(const uint32_t* __restrict__ src, uint32_t* __restrict__ host_dst, uint32_t n_words) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += gridDim.x * blockDim.x) host_dst[i] = src[i];
}
void launch_store_to_host(const void* d_src, void* h_dst, size_t bytes, hipStream_t s) {   // bytes: a multiple of 4
  const uint32_t n_words = (uint32_t)(bytes / 4);
  if (n_words == 0) return;
  const uint32_t blocks = std::min<uint32_t>(256u, (n_words + 255u) / 256u);
  hipLaunchKernelGGL(k_store_to_host, dim3(blocks), dim3(256), 0, s, static_cast<const uint32_t*>(d_src), static_cast<uint32_t*>(h_dst), n_words);
}

void launch_pack_records(const ilcc_result* d_res, uint32_t n_frames, uint32_t n_corners, uint32_t tag_base, float* d_out,
                         hipStream_t s) {
  if (n_frames) hipLaunchKernelGGL(k9_pack_records, dim3(n_frames), dim3(128), 0, s, d_res, n_corners, tag_base, d_out);
}

}  // namespace ilcc
