// K8b colourise_batch -- K8's rgblidar entry (ilcc_colourise_device, k8_project.hip) for a batch of scans, each with an image of
// its own, in THREE launches however many scans the batch holds (include/ilcc_paired.h).  A loop over ilcc_colourise_device costs,
// per scan, two launches, a stream synchronise and a host read of a page-locked counter.
//
// The scans lie back to back in d_xyzi (K0b's layout).  The host cuts every paired, non-empty scan into chunks of at most 4096
// points -- a chunk never straddles two scans, so a workgroup has ONE image -- and uploads the chunk table with a per-scan table
// (image, step) through memory the plan owns.
//   launch 1  k8b_count    one workgroup per chunk: the points that pass spaceToPlane
//   launch 2  k8b_offsets  ONE workgroup: the exclusive prefix of the chunk counts in place (256 at a time, a running carry),
//                          then out_offsets[s] = prefix[first_chunk[s]] and the total into the plan's page-locked words
//   launch 3  k8b_scatter  one workgroup per chunk: project again (the cloud comes out of L2 / Infinity Cache), rank within the
//                          workgroup, sample the scan's image, store at prefix[chunk] + rank
// K8's scatter re-sums all chunk counts in every workgroup, which is quadratic in chunks; fine for one scan's handful, not for a
// 1024-scan batch with thousands of them: that is what launch 2 is for.  No single-pass look-back variant: k8_project.hip
// records that it was measured at twice the time on this 8-XCD part.
// The projection is k8_space_to_plane.h's, compiled unfused like K8: every record is byte for byte K8's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>

#include "host_util.h"
#include "ilcc_internal.h"
#include "ilcc_paired.h"
#include "k8_space_to_plane.h"

namespace ilcc {

struct ColourChunk {
  uint32_t begin;   // first point, index into d_xyzi
  uint32_t count;   // 1 .. kProjChunk
  uint32_t scan;    // row of the scan table
  uint32_t pad;
};

struct ColourScan {
  const uint8_t* image;
  uint32_t step;
  uint32_t pad;
};

struct ColourArgs {
  const float4* pts;
  const ColourChunk* chunks;
  const ColourScan* scans;
  const uint32_t* first_chunk;   // n_scans + 1
  uint32_t* counts;              // n_chunks + 1: counts, then their exclusive prefix with the total behind it
  uint32_t n_chunks, n_scans;
  ilcc_projection cam;
  double dis;
  float4* out;
  uint32_t* out_offsets;         // page-locked, n_scans + 1
};

__global__ __launch_bounds__(kProjThreads) void k8b_count(ColourArgs a) {
  const ColourChunk c = a.chunks[blockIdx.x];
  uint32_t cnt = 0;
#pragma unroll 4
  for (uint32_t i = threadIdx.x; i < c.count; i += kProjThreads) {
    int32_t px, py;
    cnt += space_to_plane(a.cam, a.pts[c.begin + i], a.dis, px, py) ? 1u : 0u;
  }
  __shared__ uint32_t sc[17];
  const uint32_t total = block_sum<uint32_t>(cnt, sc);
  if (threadIdx.x == 0) a.counts[blockIdx.x] = total;
}

// one workgroup.  Tile by tile: inclusive scan inside each wavefront, the wavefronts' totals through LDS, a carry between tiles.
__global__ __launch_bounds__(kProjThreads) void k8b_offsets(ColourArgs a) {
  __shared__ uint32_t wave_total[kProjThreads / ILCC_WAVE];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < a.n_chunks; base += kProjThreads) {   // uniform trip count
    const uint32_t k = base + threadIdx.x;
    const uint32_t v = k < a.n_chunks ? a.counts[k] : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < ILCC_WAVE; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, ILCC_WAVE);
      if (lane_id() >= o) incl += up;
    }
    if (lane_id() == ILCC_WAVE - 1) wave_total[wave_id()] = incl;
    __syncthreads();
    uint32_t before = 0, tile = 0;
#pragma unroll
    for (int w = 0; w < kProjThreads / ILCC_WAVE; ++w) {
      const uint32_t t = wave_total[w];
      if (w < wave_id()) before += t;
      tile += t;
    }
    if (k < a.n_chunks) a.counts[k] = carry + before + incl - v;
    carry += tile;
    __syncthreads();   // wave_total is rewritten by the next tile
  }
  if (threadIdx.x == 0) a.counts[a.n_chunks] = carry;
  __syncthreads();   // the prefix, written by this workgroup, is read back below by other threads of it
  for (uint32_t s = threadIdx.x; s <= a.n_scans; s += kProjThreads) a.out_offsets[s] = a.counts[a.first_chunk[s]];
}

__global__ __launch_bounds__(kProjThreads) void k8b_scatter(ColourArgs a) {
  __shared__ uint32_t sc[17];
  const ColourChunk c = a.chunks[blockIdx.x];
  const ColourScan img = a.scans[c.scan];
  uint32_t running = a.counts[blockIdx.x];
  for (uint32_t t = 0; t < c.count; t += kProjThreads) {   // uniform trip count per workgroup
    const uint32_t i = t + threadIdx.x;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    int32_t px = 0, py = 0;
    bool keep = false;
    if (i < c.count) {
      q = a.pts[c.begin + i];
      keep = space_to_plane(a.cam, q, a.dis, px, py);
    }
    uint32_t tot;
    const uint32_t rank = block_rank(keep, sc, tot);
    if (keep) a.out[running + rank] = make_float4(q.x, q.y, q.z, __uint_as_float(sample_bgr_as_rgb(img.image, img.step, px, py)));
    running += tot;
  }
}

}  // namespace ilcc

// One allocation on each side.  Uploaded part: [chunks][scans][first_chunk]; device only: [counts]; the offsets the device writes
// are page-locked words of their own.
struct ilcc_colourise_plan {
  uint32_t max_scans = 0;
  uint64_t max_points = 0, max_chunks = 0;
  uint8_t* h_table = nullptr;     // page-locked
  uint8_t* d_table = nullptr;
  uint32_t* h_offsets = nullptr;  // page-locked, max_scans + 1, written by k8b_offsets
  hipEvent_t done = nullptr;      // behind the last launch of the plan's last call
  bool in_flight = false, accepted = false;
  uint32_t launches = 0, n_scans = 0;
  uint64_t scans_at() const { return ilcc::align256(max_chunks * sizeof(ilcc::ColourChunk)); }
  uint64_t first_at() const { return scans_at() + ilcc::align256((uint64_t)max_scans * sizeof(ilcc::ColourScan)); }
  uint64_t upload_bytes() const { return first_at() + ilcc::align256(((uint64_t)max_scans + 1) * sizeof(uint32_t)); }
  uint64_t counts_at() const { return upload_bytes(); }
  uint64_t device_bytes() const { return counts_at() + ilcc::align256((max_chunks + 1) * sizeof(uint32_t)); }
};

extern "C" {

ilcc_colourise_plan* ilcc_colourise_plan_create(uint32_t max_scans, uint64_t max_points) {
  using namespace ilcc;
  if (max_scans == 0 || max_points == 0 || max_points > 0xFFFFFFFEull) {
    fail(ILCC_BAD_ARGUMENT, "colourise plan: max_scans and max_points must be positive, max_points at most 2^32 - 2");
    return nullptr;
  }
  ilcc_colourise_plan* p = new (std::nothrow) ilcc_colourise_plan;
  if (!p) {
    fail(ILCC_IO_ERROR, "colourise plan: out of memory");
    return nullptr;
  }
  p->max_scans = max_scans;
  p->max_points = max_points;
  // every scan ends in at most one ragged chunk; the full ones are bounded by the points
  p->max_chunks = max_points / kProjChunk + std::min<uint64_t>(max_scans, max_points);
  hipError_t e = hipHostMalloc((void**)&p->h_table, p->upload_bytes(), hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc((void**)&p->h_offsets, ((uint64_t)max_scans + 1) * sizeof(uint32_t), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&p->d_table, p->device_bytes());
  if (e == hipSuccess) e = hipEventCreateWithFlags(&p->done, hipEventDisableTiming);
  if (e != hipSuccess) {
    hip_fail(e);
    ilcc_colourise_plan_destroy(p);
    return nullptr;
  }
  return p;
}

void ilcc_colourise_plan_destroy(ilcc_colourise_plan* p) {
  if (!p) return;
  if (p->in_flight) (void)hipEventSynchronize(p->done);
  if (p->done) (void)hipEventDestroy(p->done);
  if (p->d_table) (void)hipFree(p->d_table);
  if (p->h_offsets) (void)hipHostFree(p->h_offsets);
  if (p->h_table) (void)hipHostFree(p->h_table);
  delete p;
}

uint32_t ilcc_colourise_plan_launches(const ilcc_colourise_plan* p) { return p ? p->launches : 0; }

int32_t ilcc_colourise_batch_device(const void* d_xyzi, const uint64_t* offsets, uint32_t n_scans, const void* const* d_images_bgr,
                                    const uint32_t* image_steps, uint32_t n_images, const int32_t* image_of_scan,
                                    const ilcc_projection* cam, double distance_valid, void* d_xyzrgb, uint64_t cap_points,
                                    ilcc_colourise_plan* plan, void* hip_stream) {
  using namespace ilcc;
  if (!plan || !cam || (n_scans && (!offsets || !image_of_scan)) || (n_images && (!d_images_bgr || !image_steps)))
    return fail(ILCC_BAD_ARGUMENT, "colourise batch: null argument");
  if (cam->width <= 0 || cam->height <= 0) return fail(ILCC_BAD_ARGUMENT, "colourise batch: the camera's width and height must be positive");
  if (n_scans > plan->max_scans) return fail(ILCC_BAD_ARGUMENT, "colourise batch: more scans than the plan holds");

  // every refusal happens here, before the table, the copy and the launches
  uint64_t paired = 0;
  for (uint32_t s = 0; s < n_scans; ++s) {
    if (offsets[s + 1] < offsets[s]) return fail(ILCC_BAD_ARGUMENT, "colourise batch: decreasing offsets");
    const int32_t k = image_of_scan[s];
    if (k < -1 || (k >= 0 && (uint32_t)k >= n_images)) return fail(ILCC_BAD_ARGUMENT, "colourise batch: image_of_scan outside -1 .. n_images - 1");
    const uint64_t pts = offsets[s + 1] - offsets[s];
    if (k < 0 || pts == 0) continue;
    if (!d_images_bgr[k]) return fail(ILCC_BAD_ARGUMENT, "colourise batch: null argument");
    if (image_steps[k] < 3ull * (uint64_t)cam->width) return fail(ILCC_BAD_ARGUMENT, "colourise batch: image step smaller than a BGR row");
    paired += pts;
  }
  if (n_scans) {
    if (offsets[n_scans] > 0xFFFFFFFEull) return fail(ILCC_BAD_ARGUMENT, "colourise batch: more than 2^32 - 2 points");
    if (offsets[n_scans] - offsets[0] > plan->max_points) return fail(ILCC_BAD_ARGUMENT, "colourise batch: more points than the plan holds");
  }
  if (paired > cap_points) return fail(ILCC_CAPACITY, "colourise batch: the paired scans hold more points than the output");
  if (paired && (!d_xyzi || !d_xyzrgb)) return fail(ILCC_BAD_ARGUMENT, "colourise batch: null argument");

  hipError_t e;
  if (plan->in_flight) {   // the previous call still owns both copies of the table until its last launch has finished
    if ((e = hipEventSynchronize(plan->done)) != hipSuccess) return hip_fail(e);
    plan->in_flight = false;
  }
  plan->accepted = true;
  plan->n_scans = n_scans;
  plan->launches = 0;
  for (uint32_t s = 0; s <= n_scans; ++s) plan->h_offsets[s] = 0;
  if (paired == 0) return ILCC_OK;

  // chunks <= max_chunks: offsets[n] - offsets[0] <= max_points bounds the full chunks, n_scans <= max_scans the ragged ones
  ColourChunk* h_chunks = reinterpret_cast<ColourChunk*>(plan->h_table);
  ColourScan* h_scans = reinterpret_cast<ColourScan*>(plan->h_table + plan->scans_at());
  uint32_t* h_first = reinterpret_cast<uint32_t*>(plan->h_table + plan->first_at());
  uint32_t at = 0;
  for (uint32_t s = 0; s < n_scans; ++s) {
    h_first[s] = at;
    const int32_t k = image_of_scan[s];
    const uint64_t pts = offsets[s + 1] - offsets[s];
    h_scans[s] = ColourScan{nullptr, 0, 0};
    if (k < 0 || pts == 0) continue;
    h_scans[s] = ColourScan{static_cast<const uint8_t*>(d_images_bgr[k]), image_steps[k], 0};
    for (uint64_t b = 0; b < pts; b += kProjChunk)
      h_chunks[at++] = ColourChunk{(uint32_t)(offsets[s] + b), (uint32_t)std::min<uint64_t>(kProjChunk, pts - b), s, 0};
  }
  h_first[n_scans] = at;

  hipStream_t s = (hipStream_t)hip_stream;
  // one upload of the three parts (page-locked source: truly asynchronous, and the plan keeps it untouched until `done`)
  if ((e = hipMemcpyAsync(plan->d_table, plan->h_table, plan->upload_bytes(), hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e);
  plan->in_flight = true;
  ColourArgs a;
  a.pts = static_cast<const float4*>(d_xyzi);
  a.chunks = reinterpret_cast<const ColourChunk*>(plan->d_table);
  a.scans = reinterpret_cast<const ColourScan*>(plan->d_table + plan->scans_at());
  a.first_chunk = reinterpret_cast<const uint32_t*>(plan->d_table + plan->first_at());
  a.counts = reinterpret_cast<uint32_t*>(plan->d_table + plan->counts_at());
  a.n_chunks = at;
  a.n_scans = n_scans;
  a.cam = *cam;
  a.dis = distance_valid;
  a.out = static_cast<float4*>(d_xyzrgb);
  a.out_offsets = plan->h_offsets;
  hipLaunchKernelGGL(k8b_count, dim3(at), dim3(kProjThreads), 0, s, a);
  hipLaunchKernelGGL(k8b_offsets, dim3(1), dim3(kProjThreads), 0, s, a);
  hipLaunchKernelGGL(k8b_scatter, dim3(at), dim3(kProjThreads), 0, s, a);
  plan->launches = 3;
  e = hipGetLastError();
  const hipError_t er = hipEventRecord(plan->done, s);
  if (e != hipSuccess) return fail(ILCC_HIP_ERROR, std::string("k8b launch: ") + hipGetErrorString(e));
  if (er != hipSuccess) return hip_fail(er);
  return ILCC_OK;
}

int32_t ilcc_colourise_plan_finish(ilcc_colourise_plan* plan, uint64_t* out_offsets) {
  using namespace ilcc;
  if (!plan || !out_offsets) return fail(ILCC_BAD_ARGUMENT, "colourise plan: null argument");
  if (!plan->accepted) return fail(ILCC_BAD_ARGUMENT, "colourise plan: no call has been accepted yet");
  if (plan->in_flight) {
    const hipError_t e = hipEventSynchronize(plan->done);
    if (e != hipSuccess) return fail(ILCC_HIP_ERROR, std::string("k8b: ") + hipGetErrorString(e));
    plan->in_flight = false;
  }
  for (uint32_t s = 0; s <= plan->n_scans; ++s) out_offsets[s] = plan->h_offsets[s];
  return ILCC_OK;
}

}  // extern "C"
