// K8 project -- LiDAR -> image projection per point (include/ilcc_project.h):
// ImageCornersEst::spaceToPlane (/root/reference/ilcc2/src/ImageCornersEst.cpp:135-155) fused with
// the per-point colour of pcd2image (test/pcd2image.cpp:61-75, HSVtoRGB src/ImageCornersEst.cpp:373-428)
// or the image sample of rgblidar (test/rgblidar.cpp:55-74), and an order-preserving compaction.
//
// HBM-bound: 16 B read per point, 16 B written per surviving point.  Two launches like K1: count per
// 4096-point chunk, then scatter with the chunk's prefix (the second read of the cloud comes out of
// L2 / Infinity Cache for sensor-sized clouds).  The projection itself is fp64 (the reference uses
// Eigen::Vector3d / Matrix3d), compiled with -ffp-contract=off so that pixel truncation matches bit
// for bit; with three fp64 divisions per point the kernels sit near the fp64-VALU / HBM crossover.
// A single-pass variant (decoupled look-back over published chunk counts, ticketed chunk order) was
// built and measured: bit-identical but 82 us instead of 39 us for 3.7 M points -- device-scope
// atomics and acquire loads leave the XCD's own L2 on this 8-XCD part, so ~900 chained workgroups
// serialise on fabric latency.  Two passes with plain loads are the better MI355X shape.
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "host_util.h"
#include "ilcc_internal.h"
#include "ilcc_project.h"
#include "k8_space_to_plane.h"   // space_to_plane, kProjThreads, kProjChunk: shared with K8b; intensity_rgb: shared with K12b

namespace ilcc {

struct ProjArgs {
  const float4* pts;
  uint32_t n;
  ilcc_projection cam;
  double dis, lo, hi;
  const uint8_t* image;
  uint32_t image_step;
  uint32_t* counts;
  uint32_t chunks;
  void* out;
  uint32_t* total;
};

__global__ __launch_bounds__(kProjThreads) void k8_count(ProjArgs a) {
  const uint32_t beg = blockIdx.x * kProjChunk;
  const uint32_t end = (beg + kProjChunk < a.n) ? beg + kProjChunk : a.n;
  uint32_t cnt = 0;
#pragma unroll 4
  for (uint32_t i = beg + threadIdx.x; i < end; i += kProjThreads) {
    int32_t px, py;
    cnt += space_to_plane(a.cam, a.pts[i], a.dis, px, py) ? 1u : 0u;
  }
  __shared__ uint32_t sc[17];
  const uint32_t total = block_sum<uint32_t>(cnt, sc);
  if (threadIdx.x == 0) a.counts[blockIdx.x] = total;
}

template <bool SAMPLE_IMAGE>
__global__ __launch_bounds__(kProjThreads) void k8_scatter(ProjArgs a) {
  __shared__ uint32_t sc[17];
  __shared__ uint32_t s_base;
  // prefix of the chunk counts (<= a few thousand chunks): strided partial sums, then block_sum
  uint32_t part = 0, all = 0;
  for (uint32_t k = threadIdx.x; k < a.chunks; k += kProjThreads) {
    const uint32_t v = a.counts[k];
    if (k < blockIdx.x) part += v;
    all += v;
  }
  const uint32_t base0 = block_sum<uint32_t>(part, sc);
  if (blockIdx.x == 0) {
    const uint32_t tot = block_sum<uint32_t>(all, sc);
    if (threadIdx.x == 0) *a.total = tot;
  }
  if (threadIdx.x == 0) s_base = base0;
  __syncthreads();
  uint32_t running = s_base;
  const uint32_t beg = blockIdx.x * kProjChunk;
  const uint32_t end = (beg + kProjChunk < a.n) ? beg + kProjChunk : a.n;
  for (uint32_t t = beg; t < end; t += kProjThreads) {   // uniform trip count per workgroup
    const uint32_t i = t + threadIdx.x;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    int32_t px = 0, py = 0;
    bool keep = false;
    if (i < end) {
      q = a.pts[i];
      keep = space_to_plane(a.cam, q, a.dis, px, py);
    }
    uint32_t tot;
    const uint32_t rank = block_rank(keep, sc, tot);
    if (keep) {
      if (SAMPLE_IMAGE) {
        const uint32_t rgb = sample_bgr_as_rgb(a.image, a.image_step, px, py);
        reinterpret_cast<float4*>(a.out)[running + rank] = make_float4(q.x, q.y, q.z, __uint_as_float(rgb));
      } else {
        uint4 rec;
        rec.x = (uint32_t)px;
        rec.y = (uint32_t)py;
        rec.z = intensity_rgb(q.w, a.lo, a.hi);
        rec.w = i;
        reinterpret_cast<uint4*>(a.out)[running + rank] = rec;
      }
    }
    running += tot;
  }
}

namespace {
struct Scratch {
  uint32_t* counts = nullptr;
  uint32_t cap = 0;
  uint32_t* total = nullptr;
};
std::mutex g_mu;
Scratch g_scratch[16];
}  // namespace

static int32_t run_project(bool sample, const void* d_xyzi, uint32_t n, const ilcc_projection* cam, double dis, double lo,
                           double hi, const void* image, uint32_t step, void* out, uint32_t* n_out, void* stream) {
  if (!cam || !n_out || (n && (!d_xyzi || !out)) || (sample && !image) || cam->width <= 0 || cam->height <= 0)
    return fail(ILCC_BAD_ARGUMENT, "bad argument");
  if (sample && step < (uint32_t)cam->width * 3u) return fail(ILCC_BAD_ARGUMENT, "image_step smaller than a BGR row");
  *n_out = 0;
  if (n == 0) return ILCC_OK;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return no_device();
  std::lock_guard<std::mutex> lock(g_mu);
  Scratch& sc = g_scratch[dev];
  const uint32_t chunks = (n + kProjChunk - 1) / kProjChunk;
  hipError_t e = hipSuccess;
  if (sc.cap < chunks) {
    if (sc.counts) (void)hipFree(sc.counts);
    sc.counts = nullptr;
    sc.cap = 0;
    const uint32_t cap = chunks < 1024 ? 1024 : chunks;
    e = hipMalloc((void**)&sc.counts, sizeof(uint32_t) * (size_t)cap);
    if (e == hipSuccess) sc.cap = cap;
  }
  if (e == hipSuccess && !sc.total) e = hipHostMalloc((void**)&sc.total, sizeof(uint32_t));
  if (e != hipSuccess) return hip_fail(e);
  ProjArgs a;
  a.pts = (const float4*)d_xyzi;
  a.n = n;
  a.cam = *cam;
  a.dis = dis;
  a.lo = lo;
  a.hi = hi;
  a.image = (const uint8_t*)image;
  a.image_step = step;
  a.counts = sc.counts;
  a.chunks = chunks;
  a.out = out;
  a.total = sc.total;   // pinned host word, written by workgroup 0 of the scatter
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k8_count, dim3(chunks), dim3(kProjThreads), 0, s, a);
  if (sample) hipLaunchKernelGGL(k8_scatter<true>, dim3(chunks), dim3(kProjThreads), 0, s, a);
  else hipLaunchKernelGGL(k8_scatter<false>, dim3(chunks), dim3(kProjThreads), 0, s, a);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(ILCC_HIP_ERROR, std::string("k8: ") + hipGetErrorString(e));
  *n_out = *sc.total;
  return ILCC_OK;
}

}  // namespace ilcc

extern "C" int32_t ilcc_project_intensity_device(const void* d_xyzi, uint32_t n_points, const ilcc_projection* cam,
                                                 double distance_valid, double inten_low, double inten_high, void* d_hits,
                                                 uint32_t* n_hits, void* hip_stream) {
  return ilcc::run_project(false, d_xyzi, n_points, cam, distance_valid, inten_low, inten_high, nullptr, 0, d_hits, n_hits,
                           hip_stream);
}

extern "C" int32_t ilcc_colourise_device(const void* d_xyzi, uint32_t n_points, const ilcc_projection* cam,
                                         double distance_valid, const void* d_image_bgr, uint32_t image_step, void* d_xyzrgb,
                                         uint32_t* n_out, void* hip_stream) {
  return ilcc::run_project(true, d_xyzi, n_points, cam, distance_valid, 0.0, 1.0, d_image_bgr, image_step, d_xyzrgb, n_out,
                           hip_stream);
}
