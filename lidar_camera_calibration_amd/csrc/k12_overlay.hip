// K12 overlay -- replaces the cv::circle(rectifyImage, Point(x, y), 0.6, Scalar(r, g, b), 2) that pcd2image calls for every
// projected LiDAR point (/root/reference/ilcc2/test/pcd2image.cpp:59-83): K8's hits, in their order, drawn into the
// undistorted B,G,R image in device memory (include/ilcc_project.h; tests/overlay_ref.py restates it in numpy).
//
// What a sequential loop leaves in a pixel is the colour of the LAST hit whose stamp covers it, so the image is a function
// of "highest hit index per pixel" and thread order cannot show once that is computed first.  Three launches on the stream:
//   k12_clear        an owner word per pixel (the caller's scratch, 4 * width * height bytes) = 0
//   k12_walk<false>  mark: atomicMax(owner[pixel], k + 1) for every pixel of hit k's stamp that lies inside the image
//   k12_walk<true>   resolve: the same walk; hit k writes its three bytes where owner[pixel] == k + 1
// After the mark every covered pixel names exactly one hit, so the resolve has one writer per pixel: no race, no dependence
// on the scratch's earlier contents.  A thread takes one hit (one 16-byte record, loaded once) and walks the stamp, which
// travels in the kernel arguments (uniform, scalar loads); the reference's stamp has 5 pixels.  The atomics and the byte
// stores scatter by nature: 28 800 hits are 144 k of each, against which the clear (9.2 MB for 1920 x 1200, 16 bytes per
// lane per store) and three launch gaps are the larger part of the time.
#include <hip/hip_runtime.h>

#include <string>

#include "host_util.h"
#include "ilcc_internal.h"
#include "ilcc_project.h"

namespace ilcc {

constexpr int kDrawThreads = 256;
constexpr int kStampMax = 64;
constexpr uint32_t kDrawBlocksMax = 1u << 16;   // grid-stride beyond this: n_hits may be 2^32 - 2

struct Stamp {
  int32_t n;
  int8_t xy[2 * kStampMax];   // (dx, dy) pairs
};

struct alignas(4) Hit {   // ilcc_pixel_hit
  int32_t x, y;
  uint32_t rgb;           // r | g << 8 | b << 16 | pad << 24
  uint32_t index;
};

struct DrawArgs {
  uint8_t* image;
  int32_t width, height;
  int64_t stride;
  const Hit* hits;
  uint32_t n_hits;
  uint32_t* owner;   // width * height words: 0 = no hit, else (index into hits) + 1
  Stamp stamp;
};

__global__ __launch_bounds__(kDrawThreads) void k12_clear(uint32_t* owner, uint64_t n_words) {
  const bool wide = ((uintptr_t)owner & 15u) == 0;
  const uint64_t step = (uint64_t)gridDim.x * kDrawThreads * 4u;
  for (uint64_t w = ((uint64_t)blockIdx.x * kDrawThreads + threadIdx.x) * 4u; w < n_words; w += step) {
    if (wide && w + 4u <= n_words) {
      *reinterpret_cast<uint4*>(owner + w) = make_uint4(0u, 0u, 0u, 0u);
    } else {
      for (uint64_t k = w; k < w + 4u && k < n_words; ++k) owner[k] = 0u;
    }
  }
}

// pixel s of hit h's stamp: its index in the owner plane, or false when it lies outside the image.  x + dx in 64 bits:
// the coordinates are untrusted (INT32_MIN / INT32_MAX must not wrap into the image)
__device__ __forceinline__ bool stamp_pixel(const DrawArgs& a, const Hit& h, int s, int64_t& px, int64_t& py) {
  px = (int64_t)h.x + a.stamp.xy[2 * s];
  py = (int64_t)h.y + a.stamp.xy[2 * s + 1];
  return px >= 0 && px < a.width && py >= 0 && py < a.height;
}

template <bool RESOLVE>
__global__ __launch_bounds__(kDrawThreads) void k12_walk(DrawArgs a) {
  const uint64_t step = (uint64_t)gridDim.x * kDrawThreads;
  for (uint64_t k = (uint64_t)blockIdx.x * kDrawThreads + threadIdx.x; k < a.n_hits; k += step) {
    const Hit h = a.hits[k];
    const uint32_t me = (uint32_t)k + 1u;   // <= 2^32 - 2: n_hits is checked on the host
    for (int s = 0; s < a.stamp.n; ++s) {
      int64_t px, py;
      if (!stamp_pixel(a, h, s, px, py)) continue;
      uint32_t* o = a.owner + (uint64_t)py * (uint64_t)a.width + (uint64_t)px;
      if (RESOLVE) {
        if (*o != me) continue;
        uint8_t* q = a.image + py * a.stride + px * 3;
        q[0] = (uint8_t)h.rgb;           // Scalar(r, g, b) on a bgr8 image: r lands in byte 0, as in the reference
        q[1] = (uint8_t)(h.rgb >> 8);
        q[2] = (uint8_t)(h.rgb >> 16);
      } else {
        atomicMax(o, me);
      }
    }
  }
}

namespace {

// cv::circle with an int radius of 0 (0.6 truncated) and thickness 2: OpenCV 3 draws a filled circle of radius
// (2 * 2^15 + 2^15) >> 16 = 1 -- row y: x - 1 .. x + 1, rows y -+ 1: x only
constexpr int8_t kReferenceStamp[10] = {0, -1, -1, 0, 0, 0, 1, 0, 0, 1};

int32_t refuse(const std::string& what) { return fail(ILCC_BAD_ARGUMENT, "ilcc_draw_hits_device: " + what); }

}  // namespace
}  // namespace ilcc

extern "C" uint64_t ilcc_draw_hits_scratch_bytes(int32_t width, int32_t height) {
  if (width < 1 || height < 1) return 0;
  return 4ull * (uint64_t)width * (uint64_t)height;
}

extern "C" int32_t ilcc_draw_hits_device(void* d_image_bgr, int32_t width, int32_t height, int32_t stride, const void* d_hits,
                                         uint32_t n_hits, const int8_t* stamp_xy, int32_t n_stamp, void* d_scratch,
                                         void* hip_stream) {
  using namespace ilcc;
  if (!d_image_bgr || !d_scratch || (n_hits && !d_hits)) return refuse("null pointer");
  if (width < 1 || height < 1 || width > 65536 || height > 65536) return refuse("width and height must be 1 .. 65536");
  if ((int64_t)stride < 3 * (int64_t)width) return refuse("stride is shorter than a row");
  if (stamp_xy && (n_stamp < 1 || n_stamp > kStampMax)) return refuse("n_stamp must be 1 .. 64");
  if (n_hits > 0xFFFFFFFEu) return refuse("more than 2^32 - 2 hits");
  if (((uintptr_t)d_hits & 3u) || ((uintptr_t)d_scratch & 3u)) return refuse("d_hits and d_scratch must be 4-byte aligned");
  if (n_hits == 0) return ILCC_OK;

  DrawArgs a;
  a.image = (uint8_t*)d_image_bgr;
  a.width = width;
  a.height = height;
  a.stride = stride;
  a.hits = (const Hit*)d_hits;
  a.n_hits = n_hits;
  a.owner = (uint32_t*)d_scratch;
  a.stamp = Stamp{};
  a.stamp.n = stamp_xy ? n_stamp : 5;
  const int8_t* xy = stamp_xy ? stamp_xy : kReferenceStamp;
  for (int k = 0; k < 2 * a.stamp.n; ++k) a.stamp.xy[k] = xy[k];

  const uint64_t words = (uint64_t)width * (uint64_t)height;
  const uint64_t clear_blocks = (words + 4u * kDrawThreads - 1) / (4u * kDrawThreads);
  const uint64_t hit_blocks = ((uint64_t)n_hits + kDrawThreads - 1) / kDrawThreads;
  const dim3 clear_grid((uint32_t)(clear_blocks < kDrawBlocksMax ? clear_blocks : kDrawBlocksMax));
  const dim3 hit_grid((uint32_t)(hit_blocks < kDrawBlocksMax ? hit_blocks : kDrawBlocksMax));
  hipStream_t s = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(k12_clear, clear_grid, dim3(kDrawThreads), 0, s, a.owner, words);
  hipLaunchKernelGGL(k12_walk<false>, hit_grid, dim3(kDrawThreads), 0, s, a);
  hipLaunchKernelGGL(k12_walk<true>, hit_grid, dim3(kDrawThreads), 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ILCC_HIP_ERROR, std::string("k12 launch: ") + hipGetErrorString(e));
  return ILCC_OK;
}
