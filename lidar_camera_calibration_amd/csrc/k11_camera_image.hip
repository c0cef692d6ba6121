// K11 camera_image -- replaces cv_bridge::toCvCopy(msg, MONO8) and cv::undistort(image, K, d, K)
// (/root/reference/ilcc2/test/get_image_corners_bag.cpp:26,105, src/ImageCornersEst.cpp:63-66) for the
// device-resident path: pixels of a sensor_msgs/Image -> the undistorted 8-bit grayscale image K10 takes.
// The arithmetic is the one include/ilcc_camera_image.h states; tests/camera_image_ref.py restates it.
//
// ONE kernel does both jobs: no intermediate grayscale image, no stored map, no second pass over the
// frame.  Every output pixel recomputes its source coordinate in fp64 (about 35 operations, unfused:
// this file is built with -ffp-contract=off), loads its four taps, converts each to Y and blends them
// with the 15-bit integer weights.
//
// Thread-to-pixel map: a workgroup is 64 x 4 threads and covers 256 x 4 output pixels; a thread makes
// kQuad = 4 horizontally adjacent pixels and stores them as ONE dword, so a wavefront writes 256
// consecutive bytes of one output row with one store instruction.  (A byte per lane would need four
// times the store instructions for the same 256 B; 16 pixels per lane would quadruple the fp64 map
// registers a lane holds and leave a 1920-pixel row to two wavefronts.)  The dword store needs
// d_dst + row * dst_stride + 4 * column-quad to be 4-byte aligned; at misaligned bases, odd strides and
// in the row's tail the quad is stored byte by byte.  The taps are byte (or 3- / 4-byte pixel) loads at
// computed addresses: the map is smooth, so the 256 pixels of a wavefront read about 256 consecutive
// pixels of two adjacent source rows, which the L2 serves from the same few lines.  Without a camera
// the source quad sits at a known address and is loaded as dwords where that address is aligned.
//
// Bayer sources (bayer_rggb8 .. bayer_grbg8) are demosaiced in the same launch, tap by tap, by csrc/bayer_tap.h: a tap is
// D(x, y) of the header, made from the 3 x 3 raw neighbourhood of its clamped position.  With a camera the four taps of
// a pixel share ONE 4 x 4 raw window (four dword loads at any alignment, not 36 bytes); without one a thread's quad
// takes three 6-column rows (a dword and two bytes each where the address allows).  No demosaiced image exists.
//
// K11c (k11_image_to_bgr8, ilcc_image_to_bgr8_device) is the same frame kept in colour for the overlay of
// include/ilcc_overlay.h: cv_bridge::toCvCopy(msg, "bgr8") + cv::undistort (test/pcd2image.cpp:36,101).  It shares
// the map, the weights and the thread-to-pixel map; its quad is 12 bytes, stored with one 3-dword store.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "bayer_tap.h"
#include "host_util.h"
#include "ilcc_camera_image.h"
#include "ilcc_internal.h"

namespace ilcc {

constexpr int kQuad = 4;          // output pixels per thread (one dword store)
constexpr int kImgTx = 64;        // threads along x: a wavefront covers kImgTx * kQuad pixels of one row
constexpr int kImgTy = 4;         // rows per workgroup
constexpr int32_t kOutside = INT32_MIN;

struct LensArgs {
  double ifx, x0, ify, y0;   // 1 / fx, -cx / fx, 1 / fy, -cy / fy
  double fx, fy, cx, cy;
  double k1, k2, p1, p2, k3;
};

struct ImageArgs {
  const uint8_t* src;
  uint8_t* dst;
  int32_t width, height;
  int64_t src_step, dst_stride;
  LensArgs lens;
};

__device__ __forceinline__ void map_codes(const LensArgs& L, int j, int i, int32_t& iu, int32_t& iv) {
  const double x = (double)j * L.ifx + L.x0, y = (double)i * L.ify + L.y0;
  const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2.0 * x * y;
  const double kr = 1.0 + ((L.k3 * r2 + L.k2) * r2 + L.k1) * r2;
  const double u = L.fx * (x * kr + L.p1 * _2xy + L.p2 * (r2 + 2.0 * x2)) + L.cx;
  const double v = L.fy * (y * kr + L.p1 * (r2 + 2.0 * y2) + L.p2 * _2xy) + L.cy;
  const double su = u * 32.0, sv = v * 32.0;
  const bool ok = fabs(su) < 1073741824.0 && fabs(sv) < 1073741824.0;   // false for NaN and infinities too
  iu = ok ? (int32_t)rint(su) : kOutside;
  iv = ok ? (int32_t)rint(sv) : kOutside;
}

constexpr bool is_bayer(int enc) { return enc >= ILCC_ENCODING_BAYER_RGGB8 && enc <= ILCC_ENCODING_BAYER_GRBG8; }

template <int ENC>
struct Pixel {
  static constexpr bool kBayer = is_bayer(ENC);
  static constexpr int kPattern = ENC - ILCC_ENCODING_BAYER_RGGB8;   // of bayer_tap.h; meaningful when kBayer
  static constexpr int kBytes = (ENC == ILCC_ENCODING_MONO8 || kBayer) ? 1 : (ENC == ILCC_ENCODING_BGR8 || ENC == ILCC_ENCODING_RGB8) ? 3 : 4;
  static constexpr bool kBlueFirst = ENC == ILCC_ENCODING_BGR8 || ENC == ILCC_ENCODING_BGRA8;
  __device__ static __forceinline__ int32_t gray(uint32_t c0, uint32_t c1, uint32_t c2) {
    const uint32_t r = kBlueFirst ? c2 : c0, b = kBlueFirst ? c0 : c2;
    return (int32_t)((4899u * r + 9617u * c1 + 1868u * b + 8192u) >> 14);
  }
  __device__ static __forceinline__ int32_t load(const uint8_t* p) {
    if (kBytes == 1) return p[0];
    return gray(p[0], p[1], p[2]);
  }
};

// one tap of the bilinear sample; outside the source it counts as 0 (BORDER_CONSTANT), each tap on its own
template <int ENC>
__device__ __forceinline__ int32_t tap(const ImageArgs& a, int32_t x, int32_t y) {
  if ((uint32_t)x >= (uint32_t)a.width || (uint32_t)y >= (uint32_t)a.height) return 0;
  return Pixel<ENC>::load(a.src + (int64_t)y * a.src_step + (int64_t)x * Pixel<ENC>::kBytes);
}

// where output pixel (j, i) samples the source: the top-left tap and the four 15-bit weights; false: no source at all
struct Sample {
  int32_t x0, y0;
  int32_t w00, w10, w01, w11;   // taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
};

__device__ __forceinline__ bool sample_of(const LensArgs& L, int j, int i, Sample& s) {
  int32_t iu, iv;
  map_codes(L, j, i, iu, iv);
  if (iu == kOutside) return false;
  const int32_t fa = iu & 31, fb = iv & 31;
  s.x0 = iu >> 5;
  s.y0 = iv >> 5;
  s.w00 = 32 * (32 - fa) * (32 - fb);
  s.w10 = 32 * fa * (32 - fb);
  s.w01 = 32 * (32 - fa) * fb;
  s.w11 = 32 * fa * fb;
  return true;
}

__device__ __forceinline__ uint32_t blend(const Sample& s, int32_t t00, int32_t t10, int32_t t01, int32_t t11) {
  return (uint32_t)((s.w00 * t00 + s.w10 * t10 + s.w01 * t01 + s.w11 * t11 + 16384) >> 15);
}

// the four taps of a sample on a Bayer source, from one 4 x 4 raw window: Y when GRAY, else B | G << 8 | R << 16
template <int ENC, bool GRAY>
__device__ __forceinline__ void bayer_taps(const ImageArgs& a, const Sample& s, uint32_t (&t)[4]) {
  const bool any = s.x0 >= -1 && s.x0 < a.width && s.y0 >= -1 && s.y0 < a.height;
  if (!any) {
    t[0] = t[1] = t[2] = t[3] = 0;
    return;
  }
  const BayerWindow W = bayer_window(a.src, a.src_step, a.width, a.height, s.x0, s.y0);
#pragma unroll
  for (int k = 0; k < 4; ++k) t[k] = bayer_window_tap(W, a.width, a.height, Pixel<ENC>::kPattern, GRAY, s.x0 + (k & 1), s.y0 + (k >> 1));
}

// kQuad adjacent pixels of a Bayer source without a camera: three 6-column rows, then every pixel's own 3 x 3 of them
template <int ENC, bool GRAY>
__device__ __forceinline__ void bayer_quad(const ImageArgs& a, int j0, int i, int n, uint32_t (&out)[kQuad]) {
  const int lo = bayer_clamp(j0, a.width) - 1;
  const uint8_t* row = a.src + (int64_t)(bayer_clamp(i, a.height) - 1) * a.src_step;
  const uint64_t r0 = bayer_row6(row, a.width, lo), r1 = bayer_row6(row + a.src_step, a.width, lo),
                 r2 = bayer_row6(row + 2 * a.src_step, a.width, lo);
#pragma unroll
  for (int k = 0; k < kQuad; ++k)
    out[k] = k < n ? bayer_row6_pixel(r0, r1, r2, lo, a.width, a.height, Pixel<ENC>::kPattern, GRAY, j0 + k, i) : 0;
}

template <int ENC>
__device__ __forceinline__ uint32_t undistorted_pixel(const ImageArgs& a, int j, int i) {
  Sample s;
  if (!sample_of(a.lens, j, i, s)) return 0;
  if constexpr (Pixel<ENC>::kBayer) {
    uint32_t t[4];
    bayer_taps<ENC, true>(a, s, t);
    return blend(s, (int32_t)t[0], (int32_t)t[1], (int32_t)t[2], (int32_t)t[3]);
  } else {
    return blend(s, tap<ENC>(a, s.x0, s.y0), tap<ENC>(a, s.x0 + 1, s.y0), tap<ENC>(a, s.x0, s.y0 + 1), tap<ENC>(a, s.x0 + 1, s.y0 + 1));
  }
}

// the source quad of a conversion without a camera: kQuad pixels = Pixel::kBytes dwords where the address allows
template <int ENC>
__device__ __forceinline__ void source_quad(const ImageArgs& a, int j0, int i, int n, uint8_t (&bytes)[kQuad * Pixel<ENC>::kBytes]) {
  constexpr int B = Pixel<ENC>::kBytes;
  const uint8_t* p = a.src + (int64_t)i * a.src_step + (int64_t)j0 * B;
  if (n == kQuad && ((uintptr_t)p & 3u) == 0) {
#pragma unroll
    for (int k = 0; k < B; ++k) {
      const uint32_t w = reinterpret_cast<const uint32_t*>(p)[k];
      bytes[4 * k] = (uint8_t)w;
      bytes[4 * k + 1] = (uint8_t)(w >> 8);
      bytes[4 * k + 2] = (uint8_t)(w >> 16);
      bytes[4 * k + 3] = (uint8_t)(w >> 24);
    }
  } else {
#pragma unroll
    for (int k = 0; k < kQuad; ++k)
#pragma unroll
      for (int c = 0; c < B; ++c) bytes[k * B + c] = k < n ? p[k * B + c] : 0;
  }
}

template <int ENC>
__device__ __forceinline__ void converted_quad(const ImageArgs& a, int j0, int i, int n, uint32_t (&out)[kQuad]) {
  constexpr int B = Pixel<ENC>::kBytes;
  uint8_t bytes[kQuad * B];
  source_quad<ENC>(a, j0, i, n, bytes);
#pragma unroll
  for (int k = 0; k < kQuad; ++k) out[k] = B == 1 ? bytes[k] : (uint32_t)Pixel<ENC>::gray(bytes[k * B], bytes[k * B + 1], bytes[k * B + 2]);
}

template <int ENC, bool UNDISTORT>
__global__ __launch_bounds__(kImgTx* kImgTy) void k11_image_to_mono8(ImageArgs a) {
  const int j0 = (blockIdx.x * kImgTx + threadIdx.x) * kQuad;
  const int i = blockIdx.y * kImgTy + threadIdx.y;
  if (j0 >= a.width || i >= a.height) return;
  const int n = min(kQuad, a.width - j0);
  uint32_t px[kQuad];
  if (UNDISTORT) {
#pragma unroll
    for (int k = 0; k < kQuad; ++k) px[k] = k < n ? undistorted_pixel<ENC>(a, j0 + k, i) : 0;
  } else if constexpr (Pixel<ENC>::kBayer) {
    bayer_quad<ENC, true>(a, j0, i, n, px);
  } else {
    converted_quad<ENC>(a, j0, i, n, px);
  }
  uint8_t* q = a.dst + (int64_t)i * a.dst_stride + j0;
  if (n == kQuad && ((uintptr_t)q & 3u) == 0) {
    *reinterpret_cast<uint32_t*>(q) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < kQuad; ++k)
      if (k < n) q[k] = (uint8_t)px[k];
  }
}

// ---------------------------------------------------------------- K11c: the same frame as B, G, R bytes
// A pixel travels as B | G << 8 | R << 16.  The conversion permutes or replicates channels, so it commutes with the
// blend: every channel is blended on its own with the weights of sample_of.

template <int ENC>
__device__ __forceinline__ uint32_t packed_bgr(const uint8_t* p) {
  if constexpr (Pixel<ENC>::kBytes == 1) {
    return (uint32_t)p[0] * 0x010101u;
  } else {
    const uint32_t c0 = p[0], c1 = p[1], c2 = p[2];
    return Pixel<ENC>::kBlueFirst ? (c0 | (c1 << 8) | (c2 << 16)) : (c2 | (c1 << 8) | (c0 << 16));
  }
}

template <int ENC>
__device__ __forceinline__ uint32_t tap_bgr(const ImageArgs& a, int32_t x, int32_t y) {
  if ((uint32_t)x >= (uint32_t)a.width || (uint32_t)y >= (uint32_t)a.height) return 0;
  return packed_bgr<ENC>(a.src + (int64_t)y * a.src_step + (int64_t)x * Pixel<ENC>::kBytes);
}

// four packed B,G,R taps -> the packed pixel: every channel blended on its own
__device__ __forceinline__ uint32_t blend_bgr(const Sample& s, uint32_t t00, uint32_t t10, uint32_t t01, uint32_t t11) {
  uint32_t out = 0;
#pragma unroll
  for (int sh = 0; sh < 24; sh += 8)
    out |= blend(s, (int32_t)((t00 >> sh) & 255u), (int32_t)((t10 >> sh) & 255u), (int32_t)((t01 >> sh) & 255u),
                 (int32_t)((t11 >> sh) & 255u))
           << sh;
  return out;
}

template <int ENC>
__device__ __forceinline__ uint32_t undistorted_bgr(const ImageArgs& a, int j, int i) {
  Sample s;
  if (!sample_of(a.lens, j, i, s)) return 0;
  if constexpr (Pixel<ENC>::kBayer) {
    uint32_t t[4];
    bayer_taps<ENC, false>(a, s, t);
    return blend_bgr(s, t[0], t[1], t[2], t[3]);
  } else if constexpr (Pixel<ENC>::kBytes == 1) {   // three equal channels: blend one
    return blend(s, tap<ENC>(a, s.x0, s.y0), tap<ENC>(a, s.x0 + 1, s.y0), tap<ENC>(a, s.x0, s.y0 + 1), tap<ENC>(a, s.x0 + 1, s.y0 + 1)) *
           0x010101u;
  } else {
    return blend_bgr(s, tap_bgr<ENC>(a, s.x0, s.y0), tap_bgr<ENC>(a, s.x0 + 1, s.y0), tap_bgr<ENC>(a, s.x0, s.y0 + 1),
                     tap_bgr<ENC>(a, s.x0 + 1, s.y0 + 1));
  }
}

struct alignas(4) Dword3 {
  uint32_t x, y, z;
};

// The same 64 x 4 threads over 256 x 4 output pixels as k11_image_to_mono8: a thread makes kQuad adjacent pixels = 12 bytes
// and stores them as ONE 3-dword store, so a wavefront writes 768 consecutive bytes of one output row per instruction.
template <int ENC, bool UNDISTORT>
__global__ __launch_bounds__(kImgTx* kImgTy) void k11_image_to_bgr8(ImageArgs a) {
  const int j0 = (blockIdx.x * kImgTx + threadIdx.x) * kQuad;
  const int i = blockIdx.y * kImgTy + threadIdx.y;
  if (j0 >= a.width || i >= a.height) return;
  const int n = min(kQuad, a.width - j0);
  uint32_t px[kQuad];
  if (UNDISTORT) {
#pragma unroll
    for (int k = 0; k < kQuad; ++k) px[k] = k < n ? undistorted_bgr<ENC>(a, j0 + k, i) : 0;
  } else if constexpr (Pixel<ENC>::kBayer) {
    bayer_quad<ENC, false>(a, j0, i, n, px);
  } else {
    constexpr int B = Pixel<ENC>::kBytes;
    uint8_t bytes[kQuad * B];
    source_quad<ENC>(a, j0, i, n, bytes);
#pragma unroll
    for (int k = 0; k < kQuad; ++k) px[k] = packed_bgr<ENC>(bytes + k * B);
  }
  uint8_t* q = a.dst + (int64_t)i * a.dst_stride + (int64_t)j0 * 3;
  if (n == kQuad && ((uintptr_t)q & 3u) == 0) {
    Dword3 v;
    v.x = px[0] | (px[1] << 24);
    v.y = (px[1] >> 8) | (px[2] << 16);
    v.z = (px[2] >> 16) | (px[3] << 8);
    *reinterpret_cast<Dword3*>(q) = v;
  } else {
#pragma unroll
    for (int k = 0; k < kQuad; ++k)
      if (k < n) {
        q[3 * k] = (uint8_t)px[k];
        q[3 * k + 1] = (uint8_t)(px[k] >> 8);
        q[3 * k + 2] = (uint8_t)(px[k] >> 16);
      }
  }
}

__global__ __launch_bounds__(kImgTx* kImgTy) void k11_undistort_map(LensArgs lens, int32_t width, int32_t height, int32_t* iu,
                                                                    int32_t* iv) {
  const int j = blockIdx.x * kImgTx + threadIdx.x;
  const int i = blockIdx.y * kImgTy + threadIdx.y;
  if (j >= width || i >= height) return;
  int32_t cu, cv;
  map_codes(lens, j, i, cu, cv);
  const int64_t at = (int64_t)i * width + j;
  iu[at] = cu;
  iv[at] = cv;
}

namespace {

constexpr int32_t kMaxSide = 65536;

int32_t refuse(const char* entry, const std::string& what) {
  set_global_error(std::string(entry) + ": " + what);
  return ILCC_BAD_ARGUMENT;
}

// nullptr when the camera is usable for a width x height image, else what is wrong with it
const char* camera_fault(const ilcc_camera_model* c, int32_t width, int32_t height) {
  if (c->width != width || c->height != height) return "the camera's width / height differ from the image's";
  if (!std::isfinite(c->fx) || !std::isfinite(c->fy) || c->fx == 0 || c->fy == 0) return "fx and fy must be finite and non-zero";
  return nullptr;
}

LensArgs lens_of(const ilcc_camera_model* c) {
  LensArgs L;
  L.ifx = 1.0 / c->fx;
  L.x0 = -c->cx / c->fx;
  L.ify = 1.0 / c->fy;
  L.y0 = -c->cy / c->fy;
  L.fx = c->fx;
  L.fy = c->fy;
  L.cx = c->cx;
  L.cy = c->cy;
  L.k1 = c->d[0];
  L.k2 = c->d[1];
  L.p1 = c->d[2];
  L.p2 = c->d[3];
  L.k3 = c->d[4];
  return L;
}

template <int ENC, int CHANNELS>
void launch_image(const ImageArgs& a, bool undistort, dim3 grid, dim3 block, hipStream_t s) {
  if constexpr (CHANNELS == 1) {
    if (undistort) hipLaunchKernelGGL((k11_image_to_mono8<ENC, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k11_image_to_mono8<ENC, false>), grid, block, 0, s, a);
  } else {
    if (undistort) hipLaunchKernelGGL((k11_image_to_bgr8<ENC, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k11_image_to_bgr8<ENC, false>), grid, block, 0, s, a);
  }
}

// both conversions: the host checks, then one launch; CHANNELS = bytes per output pixel (1: mono8, 3: bgr8)
template <int CHANNELS>
int32_t convert_image(const char* me, const void* d_src, int32_t width, int32_t height, int32_t src_step, int32_t encoding,
                      const ilcc_camera_model* camera, void* d_dst, int32_t dst_stride, void* hip_stream) {
  if (!d_src || !d_dst) return refuse(me, "null pointer");
  if (width < 1 || height < 1 || width > kMaxSide || height > kMaxSide) return refuse(me, "width and height must be 1 .. 65536");
  int bpp;
  switch (encoding) {
    case ILCC_ENCODING_MONO8:
    case ILCC_ENCODING_BAYER_RGGB8:
    case ILCC_ENCODING_BAYER_BGGR8:
    case ILCC_ENCODING_BAYER_GBRG8:
    case ILCC_ENCODING_BAYER_GRBG8: bpp = 1; break;
    case ILCC_ENCODING_BGR8:
    case ILCC_ENCODING_RGB8: bpp = 3; break;
    case ILCC_ENCODING_BGRA8:
    case ILCC_ENCODING_RGBA8: bpp = 4; break;
    default: return refuse(me, "unknown encoding " + std::to_string(encoding));
  }
  if (is_bayer(encoding) && (width < kBayerMinSide || height < kBayerMinSide))
    return refuse(me, "a Bayer image must be at least 3 x 3 (a smaller one has no interior pixel)");
  if ((int64_t)src_step < (int64_t)width * bpp) return refuse(me, "src_step is shorter than a row");
  if ((int64_t)dst_stride < (int64_t)width * CHANNELS) return refuse(me, "dst_stride is shorter than a row");
  if (camera)
    if (const char* why = camera_fault(camera, width, height)) return refuse(me, why);
  const uintptr_t s0 = (uintptr_t)d_src, s1 = s0 + (uint64_t)(height - 1) * (uint64_t)src_step + (uint64_t)width * bpp;
  const uintptr_t t0 = (uintptr_t)d_dst, t1 = t0 + (uint64_t)(height - 1) * (uint64_t)dst_stride + (uint64_t)width * CHANNELS;
  if (s0 < t1 && t0 < s1) return refuse(me, "source and destination overlap (the kernel gathers: it cannot run in place)");

  ImageArgs a;
  a.src = (const uint8_t*)d_src;
  a.dst = (uint8_t*)d_dst;
  a.width = width;
  a.height = height;
  a.src_step = src_step;
  a.dst_stride = dst_stride;
  a.lens = camera ? lens_of(camera) : LensArgs{};
  const dim3 block(kImgTx, kImgTy);
  const dim3 grid((width + kImgTx * kQuad - 1) / (kImgTx * kQuad), (height + kImgTy - 1) / kImgTy);
  hipStream_t s = (hipStream_t)hip_stream;
  switch (encoding) {
    case ILCC_ENCODING_MONO8: launch_image<ILCC_ENCODING_MONO8, CHANNELS>(a, camera != nullptr, grid, block, s); break;
    case ILCC_ENCODING_BGR8: launch_image<ILCC_ENCODING_BGR8, CHANNELS>(a, camera != nullptr, grid, block, s); break;
    case ILCC_ENCODING_RGB8: launch_image<ILCC_ENCODING_RGB8, CHANNELS>(a, camera != nullptr, grid, block, s); break;
    case ILCC_ENCODING_BGRA8: launch_image<ILCC_ENCODING_BGRA8, CHANNELS>(a, camera != nullptr, grid, block, s); break;
    case ILCC_ENCODING_BAYER_RGGB8: launch_image<ILCC_ENCODING_BAYER_RGGB8, CHANNELS>(a, camera != nullptr, grid, block, s); break;
    case ILCC_ENCODING_BAYER_BGGR8: launch_image<ILCC_ENCODING_BAYER_BGGR8, CHANNELS>(a, camera != nullptr, grid, block, s); break;
    case ILCC_ENCODING_BAYER_GBRG8: launch_image<ILCC_ENCODING_BAYER_GBRG8, CHANNELS>(a, camera != nullptr, grid, block, s); break;
    case ILCC_ENCODING_BAYER_GRBG8: launch_image<ILCC_ENCODING_BAYER_GRBG8, CHANNELS>(a, camera != nullptr, grid, block, s); break;
    default: launch_image<ILCC_ENCODING_RGBA8, CHANNELS>(a, camera != nullptr, grid, block, s); break;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_global_error(std::string("k11 launch: ") + hipGetErrorString(e));
    return ILCC_HIP_ERROR;
  }
  return ILCC_OK;
}

}  // namespace
}  // namespace ilcc

extern "C" int32_t ilcc_image_to_mono8_device(const void* d_src, int32_t width, int32_t height, int32_t src_step,
                                              int32_t encoding, const ilcc_camera_model* camera, void* d_dst,
                                              int32_t dst_stride, void* hip_stream) {
  return ilcc::convert_image<1>("ilcc_image_to_mono8_device", d_src, width, height, src_step, encoding, camera, d_dst, dst_stride,
                                hip_stream);
}

extern "C" int32_t ilcc_image_to_bgr8_device(const void* d_src, int32_t width, int32_t height, int32_t src_step, int32_t encoding,
                                             const ilcc_camera_model* camera, void* d_dst, int32_t dst_stride, void* hip_stream) {
  return ilcc::convert_image<3>("ilcc_image_to_bgr8_device", d_src, width, height, src_step, encoding, camera, d_dst, dst_stride,
                                hip_stream);
}

extern "C" int32_t ilcc_undistort_map_device(const ilcc_camera_model* camera, int32_t* d_iu, int32_t* d_iv, void* hip_stream) {
  using namespace ilcc;
  const char* me = "ilcc_undistort_map_device";
  if (!camera || !d_iu || !d_iv) return refuse(me, "null pointer");
  if (camera->width < 1 || camera->height < 1 || camera->width > kMaxSide || camera->height > kMaxSide)
    return refuse(me, "width and height must be 1 .. 65536");
  if (const char* why = camera_fault(camera, camera->width, camera->height)) return refuse(me, why);
  const dim3 block(kImgTx, kImgTy);
  const dim3 grid((camera->width + kImgTx - 1) / kImgTx, (camera->height + kImgTy - 1) / kImgTy);
  hipLaunchKernelGGL(k11_undistort_map, grid, block, 0, (hipStream_t)hip_stream, lens_of(camera), camera->width, camera->height, d_iu,
                     d_iv);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_global_error(std::string("k11 launch: ") + hipGetErrorString(e));
    return ILCC_HIP_ERROR;
  }
  return ILCC_OK;
}
