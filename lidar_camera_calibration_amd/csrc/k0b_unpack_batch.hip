// K0b unpack_batch -- K0 for a batch of sensor_msgs/PointCloud2 messages of ANY mix of layouts and point counts, in a number of
// launches that does not grow with the batch (include/ilcc_sequence.h).  K0 needs one launch and one copy per message; its "a
// batch is one launch" covers only messages of one layout laid back to back, and real scans differ in point count.
//
// The data[] of the messages sit in one device blob; a table holds one UnpackArgs per message (source = blob + offset, destination
// = output + running point count).  A message belongs to one of five classes by K0's own rule (k0_unpack.h: tiled with point_step
// 16 / 32 / 48 / 64, or generic), and each class present is ONE launch over all its tiles.
//
// Workgroup -> (message, tile): a search in the class's prefix sum.  Per class the table lists its non-empty messages with the
// first tile of each (ascending); workgroup w takes the last entry whose first tile is <= w -- a binary search of log2(messages)
// steps on a block-uniform index, over entries that every workgroup of the launch shares.  The alternative, one (message, tile)
// row per workgroup, costs 8 bytes per 1024 points of upload and makes the table's size follow the POINT count; the prefix sum
// is 8 bytes per MESSAGE, so a plan is sized by its message count alone (a 256-scan batch: 16 KB with the per-message arguments).
// The search is ~8 dependent reads in front of a tile that moves 32 - 80 KB.
//
// HBM-bound like K0: point_step bytes read + 16 written per point.
#include <hip/hip_runtime.h>

#include <new>
#include <vector>

#include "host_util.h"
#include "ilcc_internal.h"
#include "ilcc_sequence.h"
#include "k0_unpack.h"

namespace ilcc {

constexpr int kUnpackClasses = 5;   // 0 generic, 1..4 tiled with point_step 16 * class

struct UnpackEntry {
  uint32_t first_tile;   // of this message among the tiles of its class
  uint32_t msg;          // row of the message table
};

// the last entry with first_tile <= w (entries[0].first_tile == 0, ascending, n >= 1)
__device__ __forceinline__ UnpackEntry find_entry(const UnpackEntry* __restrict__ entries, uint32_t n, uint32_t w) {
  uint32_t lo = 0, hi = n;   // invariant: entries[lo].first_tile <= w, and hi == n or entries[hi].first_tile > w
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (entries[mid].first_tile <= w) lo = mid;
    else hi = mid;
  }
  return entries[lo];
}

__global__ __launch_bounds__(kUnpackThreads) void k0b_unpack_generic(const UnpackArgs* __restrict__ msgs, const UnpackEntry* __restrict__ entries,
                                                                     uint32_t n_entries) {
  const UnpackEntry e = find_entry(entries, n_entries, blockIdx.x);
  const UnpackArgs a = msgs[e.msg];
  unpack_generic_point(a, (uint64_t)(blockIdx.x - e.first_tile) * kUnpackThreads + threadIdx.x);
}

template <int STEP16>
__global__ __launch_bounds__(kUnpackThreads) void k0b_unpack_tiled(const UnpackArgs* __restrict__ msgs, const UnpackEntry* __restrict__ entries,
                                                                   uint32_t n_entries) {
  __shared__ u32x4 tile[kUnpackTile * STEP16];
  const UnpackEntry e = find_entry(entries, n_entries, blockIdx.x);
  const UnpackArgs a = msgs[e.msg];
  unpack_tile<STEP16>(a, (uint64_t)(blockIdx.x - e.first_tile) * kUnpackTile, tile);
}

}  // namespace ilcc

// One allocation on each side: [max_msgs UnpackArgs][max_msgs UnpackEntry] -- the entries of the classes lie one class after the other
struct ilcc_unpack_plan {
  uint32_t max_msgs = 0;
  uint8_t* h_table = nullptr;   // page-locked
  uint8_t* d_table = nullptr;
  hipEvent_t done = nullptr;    // behind the last launch of the plan's last call
  bool in_flight = false;
  uint32_t launches = 0;
  uint64_t entries_at() const { return ilcc::align256((uint64_t)max_msgs * sizeof(ilcc::UnpackArgs)); }
  uint64_t bytes() const { return entries_at() + (uint64_t)max_msgs * sizeof(ilcc::UnpackEntry); }
};

extern "C" {

ilcc_unpack_plan* ilcc_unpack_plan_create(uint32_t max_msgs) {
  using namespace ilcc;
  if (max_msgs == 0) {
    fail(ILCC_BAD_ARGUMENT, "unpack plan: max_msgs must be positive");
    return nullptr;
  }
  ilcc_unpack_plan* p = new (std::nothrow) ilcc_unpack_plan;
  if (!p) {
    fail(ILCC_IO_ERROR, "unpack plan: out of memory");
    return nullptr;
  }
  p->max_msgs = max_msgs;
  hipError_t e = hipHostMalloc((void**)&p->h_table, p->bytes(), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&p->d_table, p->bytes());
  if (e == hipSuccess) e = hipEventCreateWithFlags(&p->done, hipEventDisableTiming);
  if (e != hipSuccess) {
    hip_fail(e);
    ilcc_unpack_plan_destroy(p);
    return nullptr;
  }
  return p;
}

void ilcc_unpack_plan_destroy(ilcc_unpack_plan* p) {
  if (!p) return;
  if (p->in_flight) (void)hipEventSynchronize(p->done);
  if (p->done) (void)hipEventDestroy(p->done);
  if (p->d_table) (void)hipFree(p->d_table);
  if (p->h_table) (void)hipHostFree(p->h_table);
  delete p;
}

uint32_t ilcc_unpack_plan_launches(const ilcc_unpack_plan* p) { return p ? p->launches : 0; }

int32_t ilcc_pointcloud2_unpack_batch_device(const void* d_blob, uint64_t blob_bytes, const ilcc_pointcloud2_layout* layouts,
                                             const uint64_t* src_offsets, uint32_t n_msgs, void* d_xyzi, uint64_t cap_points,
                                             uint64_t* offsets_out, ilcc_unpack_plan* plan, void* hip_stream) {
  using namespace ilcc;
  if (!plan || !offsets_out || (n_msgs && (!layouts || !src_offsets))) return fail(ILCC_BAD_ARGUMENT, "null argument");
  if (n_msgs > plan->max_msgs) return fail(ILCC_BAD_ARGUMENT, "unpack batch: more messages than the plan holds");

  // every refusal happens here, before the table, the copy and the launches
  uint64_t total = 0;
  uint64_t tiles[kUnpackClasses] = {0, 0, 0, 0, 0};
  uint32_t members[kUnpackClasses] = {0, 0, 0, 0, 0};
  for (uint32_t m = 0; m < n_msgs; ++m) {
    const ilcc_pointcloud2_layout& L = layouts[m];
    // pcl::fromROSMsg memcpy's fields: it is wrong on such data too; refuse instead
    if (L.is_bigendian) return fail(ILCC_BAD_ARGUMENT, "big-endian PointCloud2 is not supported");
    const uint64_t pts = (uint64_t)L.height * L.width;
    if (src_offsets[m] > blob_bytes || L.data_bytes > blob_bytes - src_offsets[m])
      return fail(ILCC_BAD_ARGUMENT, "unpack batch: a message's data runs past the blob");
    if (pts) {
      // what ilcc_pointcloud2_parse guarantees of a layout; a caller's own layout must not make a kernel read past its data[]
      if ((uint64_t)L.width * L.point_step > L.row_step ||
          (uint64_t)(L.height - 1) * L.row_step + (uint64_t)L.width * L.point_step > L.data_bytes)
        return fail(ILCC_BAD_ARGUMENT, "PointCloud2 steps do not fit data[]");
      for (uint32_t off : {L.off_x, L.off_y, L.off_z, L.off_intensity})
        if (off != ILCC_FIELD_ABSENT && (uint64_t)off + 4 > L.point_step) return fail(ILCC_BAD_ARGUMENT, "PointCloud2 field outside point_step");
      if (!d_blob) return fail(ILCC_BAD_ARGUMENT, "null argument");
    }
    if (pts > cap_points - total) return fail(ILCC_CAPACITY, "unpack batch: more points than the output holds");
    total += pts;
    if (pts) {
      const int c = unpack_class(L, (const uint8_t*)d_blob + src_offsets[m]);
      tiles[c] += (pts + (c ? kUnpackTile : kUnpackThreads) - 1) / (c ? kUnpackTile : kUnpackThreads);
      ++members[c];
    }
  }
  if (total && !d_xyzi) return fail(ILCC_BAD_ARGUMENT, "null argument");
  for (int c = 0; c < kUnpackClasses; ++c)
    if (tiles[c] > 0x7fffffffull) return fail(ILCC_CAPACITY, "unpack batch: more than 2^31 tiles in one layout class");

  hipError_t e;
  if (plan->in_flight) {   // the previous call still owns both copies of the table until its last launch has finished
    if ((e = hipEventSynchronize(plan->done)) != hipSuccess) return hip_fail(e);
    plan->in_flight = false;
  }
  UnpackArgs* args = reinterpret_cast<UnpackArgs*>(plan->h_table);
  UnpackEntry* entries = reinterpret_cast<UnpackEntry*>(plan->h_table + plan->entries_at());
  uint32_t class_at[kUnpackClasses], fill[kUnpackClasses], next_tile[kUnpackClasses];
  for (int c = 0, at = 0; c < kUnpackClasses; ++c) {
    class_at[c] = fill[c] = (uint32_t)at;
    next_tile[c] = 0;
    at += (int)members[c];
  }
  uint64_t run = 0;   // the destination offsets ARE the running point count: monotone by construction
  for (uint32_t m = 0; m < n_msgs; ++m) {
    const ilcc_pointcloud2_layout& L = layouts[m];
    const uint8_t* src = (const uint8_t*)d_blob + src_offsets[m];
    unpack_args_from_layout(L, src, (float4*)d_xyzi + run, &args[m]);
    offsets_out[m] = run;
    const uint64_t pts = args[m].n_points;
    if (pts) {
      const int c = unpack_class(L, src);
      entries[fill[c]++] = UnpackEntry{next_tile[c], m};
      next_tile[c] += (uint32_t)((pts + (c ? kUnpackTile : kUnpackThreads) - 1) / (c ? kUnpackTile : kUnpackThreads));
    }
    run += pts;
  }
  offsets_out[n_msgs] = run;
  plan->launches = 0;
  if (total == 0) return ILCC_OK;

  hipStream_t s = (hipStream_t)hip_stream;
  // one upload of both parts (page-locked source: truly asynchronous, and the plan keeps it untouched until `done`)
  if ((e = hipMemcpyAsync(plan->d_table, plan->h_table, plan->bytes(), hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e);
  plan->in_flight = true;
  const UnpackArgs* d_args = reinterpret_cast<const UnpackArgs*>(plan->d_table);
  const UnpackEntry* d_entries = reinterpret_cast<const UnpackEntry*>(plan->d_table + plan->entries_at());
  for (int c = 0; c < kUnpackClasses; ++c) {
    if (!members[c]) continue;
    const dim3 grid((uint32_t)tiles[c]), block(kUnpackThreads);
    const UnpackEntry* ce = d_entries + class_at[c];
    switch (c) {
      case 0: hipLaunchKernelGGL(k0b_unpack_generic, grid, block, 0, s, d_args, ce, members[c]); break;
      case 1: hipLaunchKernelGGL(k0b_unpack_tiled<1>, grid, block, 0, s, d_args, ce, members[c]); break;
      case 2: hipLaunchKernelGGL(k0b_unpack_tiled<2>, grid, block, 0, s, d_args, ce, members[c]); break;
      case 3: hipLaunchKernelGGL(k0b_unpack_tiled<3>, grid, block, 0, s, d_args, ce, members[c]); break;
      default: hipLaunchKernelGGL(k0b_unpack_tiled<4>, grid, block, 0, s, d_args, ce, members[c]); break;
    }
    ++plan->launches;
  }
  e = hipGetLastError();
  const hipError_t er = hipEventRecord(plan->done, s);
  if (e != hipSuccess) return fail(ILCC_HIP_ERROR, std::string("k0b launch: ") + hipGetErrorString(e));
  if (er != hipSuccess) return hip_fail(er);
  return ILCC_OK;
}

}  // extern "C"
