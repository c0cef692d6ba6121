// K12b overlay_batch -- pcd2image's picture (K8's intensity entry followed by K12, k8_project.hip and k12_overlay.hip) for a batch
// of scans, each drawn on a copy of an image of its own, in THREE launches however many scans the batch holds
// (include/ilcc_overlay_sequence.h).  A loop over the single-scan entries costs, per scan, five launches, a stream synchronise,
// a host read of a page-locked counter and a hit list in memory, and its pictures lie wherever the loop put them; here they come
// out as the packed array K14b reads.
//
// What the sequential loop leaves in a pixel is the colour of the LAST hit whose stamp covers it (k12_overlay.hip).  K8's
// compaction keeps point order, so "highest hit index" is "highest in-scan point index": no hit list, no count pass and no
// prefix are needed.  The scans lie back to back in d_xyzi (K0b's layout); the host cuts every paired, non-empty scan into
// chunks of at most 4096 points as K8b does -- a chunk never straddles two scans, so a workgroup has ONE canvas -- and uploads
// the chunk table with a per-scan table through memory the plan owns.
//   launch 1  k12b_prepare  grid (tiles, scan): the scan's image copied into its canvas (the 3 * width bytes of every row), its
//                           owner words (the caller's scratch, a plane per scan) zeroed, n_drawn[scan] = 0
//   launch 2  k12b_mark     one workgroup per chunk: project each point; for every stamp pixel inside the image
//                           atomicMax(owner[pixel], in-scan index + 1); the chunk's keep count through block_sum into ONE
//                           atomicAdd on n_drawn[scan]
//   launch 3  k12b_resolve  the same walk: project again, and where owner[pixel] == in-scan index + 1 compute the colour and
//                           store its three bytes.  After the mark a covered pixel names exactly one point: one writer a pixel,
//                           no race, no dependence on thread order or on the scratch's earlier contents.
// No workgroup waits for another; every loop is bounded by a count the host knows (a chunk's points, the stamp's pixels, the
// pixel groups of an image).  The projection and the colour are k8_space_to_plane.h's, compiled unfused like K8.
//
// Measured for the entry as a whole (tools/dev_overlay_sequence_timing.py): 32 scans x 28 800 points take 0.49 ms
// on 1920 x 1200 images and 0.29 ms on 702 x 629, against 2.10 and 1.89 ms for the loop over the single-scan entries.  The split
// between the passes has NOT been measured; what bounds each of them is reasoning:
//   prepare   streams: per paired scan 3wh bytes read, 3wh + 4wh written (1920 x 1200: 6.9 + 16.1 MB); HBM-bound, and by far
//             the most bytes of the three.
//   mark      per kept point 16 bytes read and one 4-byte atomic per stamp pixel (5 with the reference's stamp; 28 800 points
//             are 144 k atomics).  The owner plane of one scan (9.2 MB at 1920 x 1200) does not fit one XCD's 4 MB L2, and a
//             device-scope atomic is performed beyond it anyway: every one is a fabric round trip to memory-side cache, and
//             the lines it touches are dropped from the XCD's L2.  Neighbouring scan lines hit neighbouring pixels, so the
//             atomics of a wavefront fall into few 128-byte lines.  Bound by the rate of scattered atomics, not by bytes or
//             by the fp64 projection (three divisions a point).
//   resolve   per kept point one 4-byte owner load per stamp pixel -- a miss in L2, since the mark's atomics left nothing
//             there, served by Infinity Cache where the planes of the batch fit its 256 MB -- and three byte stores where it
//             wins, each a partial write of a line.  Bound by the latency of those scattered loads, which only occupancy
//             hides: 256 threads, no LDS beyond block_sum's, so several workgroups a CU.
// With few points a scan the three launch gaps and the prepare are the larger part of the time, as in K12.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>

#include "host_util.h"
#include "ilcc_internal.h"
#include "ilcc_overlay_sequence.h"
#include "k8_space_to_plane.h"

namespace ilcc {

constexpr int kOverlayStampMax = 64;
constexpr uint32_t kPrepareTilesMax = 1024;   // per scan; grid-stride beyond this
constexpr uint32_t kGroupPixels = 4;          // pixels a thread of the prepare takes at a time: 12 image bytes, 16 owner bytes

struct OverlayChunk {
  uint32_t begin;   // first point, index into d_xyzi
  uint32_t count;   // 1 .. kProjChunk
  uint32_t scan;    // row of the scan table
  uint32_t first;   // in-scan index of the chunk's first point
};

struct OverlayScan {
  const uint8_t* image;   // nullptr: unpaired, nothing of the scan is touched
  uint32_t step;
  uint32_t pad;
};

struct OverlayStamp {
  int32_t n;
  int8_t xy[2 * kOverlayStampMax];   // (dx, dy) pairs
};

struct OverlayArgs {
  const float4* pts;
  const OverlayChunk* chunks;
  const OverlayScan* scans;
  uint32_t* n_drawn;        // n_scans, device
  uint8_t* canvas;
  uint64_t canvas_pitch;
  int64_t canvas_stride;
  uint8_t* owner;           // plane s at owner + s * owner_pitch
  uint64_t owner_pitch;     // bytes, a multiple of 16
  uint32_t groups_per_row;  // ceil(width / kGroupPixels)
  uint32_t n_groups;        // groups_per_row * height
  ilcc_projection cam;
  double dis, lo, hi;
  OverlayStamp stamp;
};

__global__ __launch_bounds__(kProjThreads) void k12b_prepare(OverlayArgs a) {
  const uint32_t s = blockIdx.y;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.n_drawn[s] = 0u;
  const OverlayScan sc = a.scans[s];
  if (!sc.image) return;
  uint8_t* canvas = a.canvas + (uint64_t)s * a.canvas_pitch;
  uint32_t* owner = reinterpret_cast<uint32_t*>(a.owner + (uint64_t)s * a.owner_pitch);
  const uint32_t w = (uint32_t)a.cam.width;
  const uint32_t step = gridDim.x * kProjThreads;
  for (uint32_t g = blockIdx.x * kProjThreads + threadIdx.x; g < a.n_groups; g += step) {   // n_groups < 2^31: the host checks
    const uint32_t y = g / a.groups_per_row, x0 = (g - y * a.groups_per_row) * kGroupPixels;
    const uint32_t n = w - x0 < kGroupPixels ? w - x0 : kGroupPixels;
    const uint8_t* src = sc.image + (uint64_t)y * sc.step + 3u * x0;
    uint8_t* dst = canvas + (int64_t)y * a.canvas_stride + 3u * x0;
    uint32_t* o = owner + (uint64_t)y * w + x0;
    if (n == kGroupPixels && (((uintptr_t)src | (uintptr_t)dst) & 3u) == 0) {
      const uint32_t b0 = reinterpret_cast<const uint32_t*>(src)[0], b1 = reinterpret_cast<const uint32_t*>(src)[1],
                     b2 = reinterpret_cast<const uint32_t*>(src)[2];
      reinterpret_cast<uint32_t*>(dst)[0] = b0;
      reinterpret_cast<uint32_t*>(dst)[1] = b1;
      reinterpret_cast<uint32_t*>(dst)[2] = b2;
    } else {
      for (uint32_t k = 0; k < 3u * n; ++k) dst[k] = src[k];
    }
    if (n == kGroupPixels && ((uintptr_t)o & 15u) == 0) {
      *reinterpret_cast<uint4*>(o) = make_uint4(0u, 0u, 0u, 0u);
    } else {
      for (uint32_t k = 0; k < n; ++k) o[k] = 0u;
    }
  }
}

// pixel t of the stamp around (x, y): false when it lies outside the image.  x + dx in 64 bits, as K12 adds them
__device__ __forceinline__ bool stamp_pixel(const OverlayArgs& a, int32_t x, int32_t y, int t, int64_t& px, int64_t& py) {
  px = (int64_t)x + a.stamp.xy[2 * t];
  py = (int64_t)y + a.stamp.xy[2 * t + 1];
  return px >= 0 && px < a.cam.width && py >= 0 && py < a.cam.height;
}

template <bool RESOLVE>
__global__ __launch_bounds__(kProjThreads) void k12b_walk(OverlayArgs a) {
  const OverlayChunk c = a.chunks[blockIdx.x];
  uint32_t* owner = reinterpret_cast<uint32_t*>(a.owner + (uint64_t)c.scan * a.owner_pitch);
  uint8_t* canvas = a.canvas + (uint64_t)c.scan * a.canvas_pitch;
  uint32_t cnt = 0;
  for (uint32_t i = threadIdx.x; i < c.count; i += kProjThreads) {
    const float4 q = a.pts[c.begin + i];
    int32_t x, y;
    if (!space_to_plane(a.cam, q, a.dis, x, y)) continue;
    ++cnt;
    const uint32_t me = c.first + i + 1u;   // <= 2^32 - 2: the points are checked on the host
    uint32_t rgb = 0;
    bool coloured = false;
    for (int t = 0; t < a.stamp.n; ++t) {
      int64_t px, py;
      if (!stamp_pixel(a, x, y, t, px, py)) continue;
      uint32_t* o = owner + (uint64_t)py * (uint64_t)a.cam.width + (uint64_t)px;
      if (RESOLVE) {
        if (*o != me) continue;
        if (!coloured) {
          rgb = intensity_rgb(q.w, a.lo, a.hi);
          coloured = true;
        }
        uint8_t* p = canvas + py * a.canvas_stride + px * 3;
        p[0] = (uint8_t)rgb;           // Scalar(r, g, b) on a bgr8 image: r lands in byte 0, as in the reference
        p[1] = (uint8_t)(rgb >> 8);
        p[2] = (uint8_t)(rgb >> 16);
      } else {
        atomicMax(o, me);
      }
    }
  }
  if (!RESOLVE) {
    __shared__ uint32_t sm[17];
    const uint32_t total = block_sum<uint32_t>(cnt, sm);
    if (threadIdx.x == 0 && total) atomicAdd(a.n_drawn + c.scan, total);
  }
}

namespace {

// cv::circle with an int radius of 0 and thickness 2, as k12_overlay.hip states it
constexpr int8_t kReferenceStamp[10] = {0, -1, -1, 0, 0, 0, 1, 0, 0, 1};

int32_t refuse(const std::string& what) { return fail(ILCC_BAD_ARGUMENT, "overlay batch: " + what); }

uint64_t owner_plane_bytes(int32_t width, int32_t height) { return (4ull * (uint64_t)width * (uint64_t)height + 15u) & ~(uint64_t)15u; }

}  // namespace
}  // namespace ilcc

// One allocation on each side.  Uploaded part: [chunks][scans]; device only: [n_drawn]; the counts come back into page-locked
// words of their own.
struct ilcc_overlay_plan {
  uint32_t max_scans = 0;
  uint64_t max_points = 0, max_chunks = 0;
  uint8_t* h_table = nullptr;     // page-locked
  uint8_t* d_table = nullptr;
  uint32_t* h_drawn = nullptr;    // page-locked, max_scans
  hipEvent_t done = nullptr;      // behind the last launch and copy of the plan's last call
  bool in_flight = false, accepted = false;
  uint32_t launches = 0, n_scans = 0;
  uint64_t scans_at() const { return ilcc::align256(max_chunks * sizeof(ilcc::OverlayChunk)); }
  uint64_t upload_bytes() const { return scans_at() + ilcc::align256((uint64_t)max_scans * sizeof(ilcc::OverlayScan)); }
  uint64_t drawn_at() const { return upload_bytes(); }
  uint64_t device_bytes() const { return drawn_at() + ilcc::align256((uint64_t)max_scans * sizeof(uint32_t)); }
};

extern "C" {

ilcc_overlay_plan* ilcc_overlay_plan_create(uint32_t max_scans, uint64_t max_points) {
  using namespace ilcc;
  if (max_scans == 0 || max_scans > 65535u || max_points == 0 || max_points > 0xFFFFFFFEull) {
    fail(ILCC_BAD_ARGUMENT, "overlay plan: max_scans must be 1 .. 65535 and max_points 1 .. 2^32 - 2");
    return nullptr;
  }
  ilcc_overlay_plan* p = new (std::nothrow) ilcc_overlay_plan;
  if (!p) {
    fail(ILCC_IO_ERROR, "overlay plan: out of memory");
    return nullptr;
  }
  p->max_scans = max_scans;
  p->max_points = max_points;
  // every scan ends in at most one ragged chunk; the full ones are bounded by the points
  p->max_chunks = max_points / kProjChunk + std::min<uint64_t>(max_scans, max_points);
  hipError_t e = hipHostMalloc((void**)&p->h_table, p->upload_bytes(), hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc((void**)&p->h_drawn, (uint64_t)max_scans * sizeof(uint32_t), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&p->d_table, p->device_bytes());
  if (e == hipSuccess) e = hipEventCreateWithFlags(&p->done, hipEventDisableTiming);
  if (e != hipSuccess) {
    hip_fail(e);
    ilcc_overlay_plan_destroy(p);
    return nullptr;
  }
  return p;
}

void ilcc_overlay_plan_destroy(ilcc_overlay_plan* p) {
  if (!p) return;
  if (p->in_flight) (void)hipEventSynchronize(p->done);
  if (p->done) (void)hipEventDestroy(p->done);
  if (p->d_table) (void)hipFree(p->d_table);
  if (p->h_drawn) (void)hipHostFree(p->h_drawn);
  if (p->h_table) (void)hipHostFree(p->h_table);
  delete p;
}

uint32_t ilcc_overlay_plan_launches(const ilcc_overlay_plan* p) { return p ? p->launches : 0; }

uint64_t ilcc_overlay_batch_scratch_bytes(int32_t width, int32_t height, uint32_t n_scans) {
  if (width < 1 || height < 1 || width > 65536 || height > 65536) return 0;
  return ilcc::owner_plane_bytes(width, height) * (uint64_t)n_scans;
}

int32_t ilcc_overlay_batch_device(const ilcc_overlay_batch_job* job) {
  using namespace ilcc;
  if (!job) return refuse("null argument");
  const ilcc_overlay_batch_job& J = *job;
  ilcc_overlay_plan* plan = J.plan;
  if (!plan || !J.cam || (J.n_scans && (!J.offsets || !J.image_of_scan)) || (J.n_images && (!J.d_images_bgr || !J.image_steps)))
    return refuse("null argument");
  const int32_t w = J.cam->width, h = J.cam->height;
  if (w < 1 || h < 1 || w > 65536 || h > 65536) return refuse("the camera's width and height must be 1 .. 65536");
  if (J.stamp_xy && (J.n_stamp < 1 || J.n_stamp > kOverlayStampMax)) return refuse("n_stamp must be 1 .. 64");
  if ((int64_t)J.canvas_stride < 3 * (int64_t)w) return refuse("canvas_stride is shorter than a row");
  if (J.canvas_pitch < (uint64_t)J.canvas_stride * (uint64_t)(h - 1) + 3ull * (uint64_t)w) return refuse("canvas_pitch is short of a canvas");
  if (J.n_scans > plan->max_scans) return refuse("more scans than the plan holds");

  // every refusal happens here, before the table, the copy and the launches
  uint64_t paired_points = 0;
  uint32_t paired_scans = 0;
  for (uint32_t s = 0; s < J.n_scans; ++s) {
    if (J.offsets[s + 1] < J.offsets[s]) return refuse("decreasing offsets");
    const int32_t k = J.image_of_scan[s];
    if (k < -1 || (k >= 0 && (uint32_t)k >= J.n_images)) return refuse("image_of_scan outside -1 .. n_images - 1");
    if (k < 0) continue;
    if (!J.d_images_bgr[k]) return refuse("null argument");
    if (J.image_steps[k] < 3ull * (uint64_t)w) return refuse("image step smaller than a BGR row");
    ++paired_scans;
    paired_points += J.offsets[s + 1] - J.offsets[s];
  }
  if (J.n_scans) {
    if (J.offsets[J.n_scans] > 0xFFFFFFFEull) return refuse("more than 2^32 - 2 points");
    if (J.offsets[J.n_scans] - J.offsets[0] > plan->max_points) return refuse("more points than the plan holds");
  }
  const uint64_t plane = owner_plane_bytes(w, h);
  if (paired_scans) {
    if (!J.d_canvas || !J.d_scratch) return refuse("null argument");
    if (J.scratch_bytes < plane * J.n_scans) return refuse("scratch_bytes is less than ilcc_overlay_batch_scratch_bytes");
    if ((uintptr_t)J.d_scratch & 15u) return refuse("d_scratch must be 16-byte aligned");
  }
  if (paired_points && !J.d_xyzi) return refuse("null argument");

  hipError_t e;
  if (plan->in_flight) {   // the previous call still owns both copies of the table and the counts until its last copy has finished
    if ((e = hipEventSynchronize(plan->done)) != hipSuccess) return hip_fail(e);
    plan->in_flight = false;
  }
  plan->accepted = true;
  plan->n_scans = J.n_scans;
  plan->launches = 0;
  for (uint32_t s = 0; s < J.n_scans; ++s) plan->h_drawn[s] = 0;
  if (paired_scans == 0) return ILCC_OK;

  // chunks <= max_chunks: offsets[n] - offsets[0] <= max_points bounds the full chunks, n_scans <= max_scans the ragged ones
  OverlayChunk* h_chunks = reinterpret_cast<OverlayChunk*>(plan->h_table);
  OverlayScan* h_scans = reinterpret_cast<OverlayScan*>(plan->h_table + plan->scans_at());
  uint32_t at = 0;
  for (uint32_t s = 0; s < J.n_scans; ++s) {
    const int32_t k = J.image_of_scan[s];
    h_scans[s] = OverlayScan{nullptr, 0, 0};
    if (k < 0) continue;
    h_scans[s] = OverlayScan{static_cast<const uint8_t*>(J.d_images_bgr[k]), J.image_steps[k], 0};
    const uint64_t pts = J.offsets[s + 1] - J.offsets[s];
    for (uint64_t b = 0; b < pts; b += kProjChunk)
      h_chunks[at++] = OverlayChunk{(uint32_t)(J.offsets[s] + b), (uint32_t)std::min<uint64_t>(kProjChunk, pts - b), s, (uint32_t)b};
  }

  hipStream_t st = (hipStream_t)J.hip_stream;
  // one upload of both parts (page-locked source: truly asynchronous, and the plan keeps it untouched until `done`)
  if ((e = hipMemcpyAsync(plan->d_table, plan->h_table, plan->upload_bytes(), hipMemcpyHostToDevice, st)) != hipSuccess) return hip_fail(e);
  plan->in_flight = true;
  OverlayArgs a;
  a.pts = static_cast<const float4*>(J.d_xyzi);
  a.chunks = reinterpret_cast<const OverlayChunk*>(plan->d_table);
  a.scans = reinterpret_cast<const OverlayScan*>(plan->d_table + plan->scans_at());
  a.n_drawn = reinterpret_cast<uint32_t*>(plan->d_table + plan->drawn_at());
  a.canvas = static_cast<uint8_t*>(J.d_canvas);
  a.canvas_pitch = J.canvas_pitch;
  a.canvas_stride = J.canvas_stride;
  a.owner = static_cast<uint8_t*>(J.d_scratch);
  a.owner_pitch = plane;
  a.groups_per_row = ((uint32_t)w + kGroupPixels - 1) / kGroupPixels;
  a.n_groups = a.groups_per_row * (uint32_t)h;   // <= 16384 * 65536 = 2^30
  a.cam = *J.cam;
  a.dis = J.distance_valid;
  a.lo = J.inten_low;
  a.hi = J.inten_high;
  a.stamp = OverlayStamp{};
  a.stamp.n = J.stamp_xy ? J.n_stamp : 5;
  const int8_t* xy = J.stamp_xy ? J.stamp_xy : kReferenceStamp;
  for (int k = 0; k < 2 * a.stamp.n; ++k) a.stamp.xy[k] = xy[k];

  const uint32_t tiles = std::min<uint32_t>((a.n_groups + kProjThreads - 1) / kProjThreads, kPrepareTilesMax);
  hipLaunchKernelGGL(k12b_prepare, dim3(tiles, J.n_scans), dim3(kProjThreads), 0, st, a);
  plan->launches = 1;
  if (at) {
    hipLaunchKernelGGL(k12b_walk<false>, dim3(at), dim3(kProjThreads), 0, st, a);
    hipLaunchKernelGGL(k12b_walk<true>, dim3(at), dim3(kProjThreads), 0, st, a);
    plan->launches = 3;
  }
  e = hipGetLastError();
  hipError_t ec = hipSuccess;
  if (at) ec = hipMemcpyAsync(plan->h_drawn, a.n_drawn, (uint64_t)J.n_scans * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
  const hipError_t er = hipEventRecord(plan->done, st);
  if (e != hipSuccess) return fail(ILCC_HIP_ERROR, std::string("k12b launch: ") + hipGetErrorString(e));
  if (ec != hipSuccess) return hip_fail(ec);
  if (er != hipSuccess) return hip_fail(er);
  return ILCC_OK;
}

int32_t ilcc_overlay_plan_finish(ilcc_overlay_plan* plan, uint32_t* n_drawn_out) {
  using namespace ilcc;
  if (!plan || !n_drawn_out) return fail(ILCC_BAD_ARGUMENT, "overlay plan: null argument");
  if (!plan->accepted) return fail(ILCC_BAD_ARGUMENT, "overlay plan: no call has been accepted yet");
  if (plan->in_flight) {
    const hipError_t e = hipEventSynchronize(plan->done);
    if (e != hipSuccess) return fail(ILCC_HIP_ERROR, std::string("k12b: ") + hipGetErrorString(e));
    plan->in_flight = false;
  }
  for (uint32_t s = 0; s < plan->n_scans; ++s) n_drawn_out[s] = plan->h_drawn[s];
  return ILCC_OK;
}

}  // extern "C"
