// K10 image corners -- libcbdetect's findCorners (libcbdetect/matching/findCorners.m) on the GPU
// (include/ilcc_image_corners.h).  Five launches on the caller's stream:
//
//   k10_minmax        grid-stride min / max of the 8-bit image (findCorners.m:45-49)
//   k10_gradients     one thread per pixel: integer numerators of img_du / img_dv (:31-37), int16
//   k10_likelihood    16 x 16 outputs per workgroup over a 40 x 40 LDS tile of (I - min); every tap of
//                     the six template classes (:51-85, createCorrelationPatch.m) from constant
//                     memory, fp32 accumulation, one scale by 1 / (max - min) at the end
//   k10_nms           one thread per scan block of nonMaximumSuppression.m (n = 3, margin 5),
//                     atomic append of the block id; the host sorts the ids into scan order
//   k10_refine_score  one wavefront per candidate, fp64: edgeOrientations + findModesMeanShift
//                     (refineCorners.m:125-175, findModesMeanShift.m), the orientation and position
//                     refinement (refineCorners.m:35-120) and scoreCorners.m at radii 4 / 8 / 12
//
// The stage bodies live in k10_stages.h, which the batch kernels (k10b_image_corners_batch.hip) call too.
// The likelihood is linear in (I - min), so it runs on integer pixel values and is scaled once.  Angle
// and weight are formed per window pixel in fp64 from the int16 numerators, as im2double does
// (I / 255).  The file is compiled with -ffp-contract=off like the other fp64 stage kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "host_util.h"
#include "ilcc_image_corners.h"
#include "ilcc_internal.h"
#include "k10_stages.h"   // the stage bodies, shared with the batch kernels (k10b_image_corners_batch.hip)

namespace ilcc {

namespace {

__global__ void k10_minmax(const uint8_t* img, int w, int h, int stride, uint32_t* mm) { minmax_body(img, w, h, stride, mm, blockIdx.x, gridDim.x); }

__global__ void k10_gradients(const uint8_t* img, int w, int h, int stride, short2* grad) {
  gradients_body(img, w, h, stride, grad, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y * blockDim.y + threadIdx.y);
}

__global__ __launch_bounds__(kTile* kTile) void k10_likelihood(const uint8_t* img, int w, int h, int stride, const uint32_t* mm,
                                                              float* L) {
  __shared__ float tile[kTileIn][kTileIn];
  likelihood_body(img, w, h, stride, mm, L, blockIdx.x, blockIdx.y, tile);
}

// one thread per scan block; atomic append of the block id, which the host sorts into scan order
__global__ void k10_nms(const float* L, int w, int h, int nbx, int nby, uint32_t* count, int4* out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nbx * nby) return;
  int maxi, maxj;
  if (!nms_block(L, w, h, nby, b, maxi, maxj)) return;
  const uint32_t slot = atomicAdd(count, 1u);
  out[slot] = make_int4(b, maxi, maxj, 0);   // slot < nbx * nby: at most one entry per block
}

struct RefineArgs {
  RefineImage image;
  const int2* cand;   // 1-based (u, v), scan order
  int n;
  Record* out;
};

__global__ __launch_bounds__(kWave) void k10_refine_score(RefineArgs A) {
  const int k = blockIdx.x;
  if (k >= A.n) return;
  refine_score_body(A.image, A.cand[k].x, A.cand[k].y, &A.out[k]);
}

int32_t hip_fail(const char* what, hipError_t e) { return k10_hip_fail(what, e); }

}  // namespace

int32_t image_corners(const void* d_image, int32_t w, int32_t h, int32_t stride, ilcc_image_corner* corners, int32_t capacity,
                      int32_t* n_corners, ilcc_image_corner_stages* stages, void* stream) {
  if (!d_image || !n_corners || capacity < 0 || (capacity > 0 && !corners)) {
    set_global_error("ilcc_image_corners_device: null image, output or count");
    return ILCC_BAD_ARGUMENT;
  }
  if (w < kMinSide || h < kMinSide) {
    set_global_error("ilcc_image_corners_device: image " + std::to_string(w) + " x " + std::to_string(h) +
                     " is smaller than " + std::to_string(kMinSide) + " px a side (2 x 12 + 2 x 5)");
    return ILCC_BAD_ARGUMENT;
  }
  if (stride < w) {
    set_global_error("ilcc_image_corners_device: stride " + std::to_string(stride) + " below width " + std::to_string(w));
    return ILCC_BAD_ARGUMENT;
  }
  *n_corners = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return no_device();
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  const int32_t taps = ensure_taps(dev);
  if (taps != ILCC_OK) return taps;
  const int nbx = nms_blocks(w), nby = nms_blocks(h);
  const size_t npx = (size_t)w * h, nblk = (size_t)nbx * nby;
  // one allocation: grad | L | cand | mm + count
  const size_t off_L = ((npx * sizeof(short2)) + 255) & ~(size_t)255;
  const size_t off_c = off_L + (((npx * sizeof(float)) + 255) & ~(size_t)255);
  const size_t off_m = off_c + ((nblk * sizeof(int4) + 255) & ~(size_t)255);
  const size_t total = off_m + 256;
  char* buf = nullptr;
  e = hipMalloc((void**)&buf, total);
  if (e != hipSuccess) return hip_fail("scratch", e);
  short2* grad = (short2*)buf;
  float* L = (stages && stages->d_likelihood) ? stages->d_likelihood : (float*)(buf + off_L);
  int4* cand = (int4*)(buf + off_c);
  uint32_t* mm = (uint32_t*)(buf + off_m);   // [0] min, [1] max, [2] candidate count
  Record* d_rec = nullptr;
  hipEvent_t ev[5] = {};
  const bool timed = stages != nullptr;
  int32_t st = ILCC_OK;
  std::vector<int4> hc;
  std::vector<Record> rec;
  uint32_t hmm[3] = {0, 0, 0};
  const uint32_t init[3] = {0xFFFFFFFFu, 0u, 0u};
  if (timed)
    for (auto& x : ev) (void)hipEventCreate(&x);
  if (timed) (void)hipEventRecord(ev[0], s);
  e = hipMemcpyAsync(mm, init, sizeof(init), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    const int blocks = (int)std::min<size_t>((npx + 255) / 256, 1024);
    hipLaunchKernelGGL(k10_minmax, dim3(blocks), dim3(256), 0, s, (const uint8_t*)d_image, w, h, stride, mm);
    hipLaunchKernelGGL(k10_gradients, dim3((w + 31) / 32, (h + 7) / 8), dim3(32, 8), 0, s, (const uint8_t*)d_image, w, h,
                       stride, grad);
    if (timed) (void)hipEventRecord(ev[1], s);
    hipLaunchKernelGGL(k10_likelihood, dim3((w + kTile - 1) / kTile, (h + kTile - 1) / kTile), dim3(kTile, kTile), 0, s,
                       (const uint8_t*)d_image, w, h, stride, (const uint32_t*)mm, L);
    if (timed) (void)hipEventRecord(ev[2], s);
    if (nblk) hipLaunchKernelGGL(k10_nms, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, s, (const float*)L, w, h, nbx, nby, mm + 2, cand);
    if (timed) (void)hipEventRecord(ev[3], s);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(hmm, mm, sizeof(hmm), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess && hmm[2] > nblk) e = hipErrorUnknown;   // cannot happen: one entry per block
  const uint32_t nc = hmm[2];
  if (e == hipSuccess && nc) {
    hc.resize(nc);
    e = hipMemcpyAsync(hc.data(), cand, sizeof(int4) * nc, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  }
  if (e == hipSuccess && nc) {
    // scan order of nonMaximumSuppression.m: block id = bx * nby + by (u outer, v inner)
    std::sort(hc.begin(), hc.end(), [](const int4& a, const int4& b) { return a.x < b.x; });
    std::vector<int2> uv(nc);
    for (uint32_t i = 0; i < nc; ++i) uv[i] = make_int2(hc[i].y, hc[i].z);
    e = hipMalloc((void**)&d_rec, sizeof(Record) * nc);
    // reuse the candidate buffer for the sorted (u, v) list: nc int2 fit in nc int4
    if (e == hipSuccess) e = hipMemcpyAsync(cand, uv.data(), sizeof(int2) * nc, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
      RefineArgs A;
      A.image.img = (const uint8_t*)d_image;
      A.image.grad = grad;
      A.image.mm = mm;
      A.cand = (const int2*)cand;
      A.image.w = w;
      A.image.h = h;
      A.image.stride = stride;
      A.n = (int)nc;
      A.out = d_rec;
      hipLaunchKernelGGL(k10_refine_score, dim3(nc), dim3(kWave), 0, s, A);
      e = hipGetLastError();
    }
    if (timed) (void)hipEventRecord(ev[4], s);
    rec.resize(nc);
    if (e == hipSuccess) e = hipMemcpyAsync(rec.data(), d_rec, sizeof(Record) * nc, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  } else if (timed && e == hipSuccess) {
    (void)hipEventRecord(ev[4], s);
    e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) st = hip_fail("launch", e);
  if (st == ILCC_OK && timed) {
    for (int i = 0; i < 4; ++i) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
      stages->ms[i] = ms;
    }
    stages->n_candidates = (int32_t)nc;
    for (uint32_t i = 0; i < nc && (int32_t)i < stages->capacity; ++i) {
      if (stages->candidates) {
        stages->candidates[2 * i] = hc[i].y;
        stages->candidates[2 * i + 1] = hc[i].z;
      }
      if (stages->refined) {
        ilcc_image_corner& o = stages->refined[i];
        o.u = rec[i].p[0]; o.v = rec[i].p[1];
        o.v1[0] = rec[i].v1[0]; o.v1[1] = rec[i].v1[1]; o.v2[0] = rec[i].v2[0]; o.v2[1] = rec[i].v2[1];
        o.score = rec[i].score;
      }
    }
  }
  if (st == ILCC_OK) {
    const int32_t cnt = finish_corners(rec.data(), nc, corners, capacity);   // findCorners.m:97-125
    *n_corners = cnt;
    if (cnt > capacity) {
      set_global_error("ilcc_image_corners_device: " + std::to_string(cnt) + " corners exceed capacity " + std::to_string(capacity));
      st = ILCC_CAPACITY;
    }
  }
  if (timed)
    for (auto& x : ev) (void)hipEventDestroy(x);
  if (d_rec) (void)hipFree(d_rec);
  (void)hipFree(buf);
  return st;
}

}  // namespace ilcc

extern "C" int32_t ilcc_image_corners_device(const void* d_image, int32_t width, int32_t height, int32_t stride,
                                             ilcc_image_corner* corners, int32_t capacity, int32_t* n_corners,
                                             ilcc_image_corner_stages* stages, void* hip_stream) {
  return ilcc::image_corners(d_image, width, height, stride, corners, capacity, n_corners, stages, hip_stream);
}
