// K10b image corners of a BATCH of images -- findCorners on n equal-sized 8-bit images in at most eight launches
// (include/ilcc_image_sequence.h), whatever n is.  The stage bodies are K10's own (k10_stages.h); what is new here is
// the image as a grid dimension, the plan that owns every buffer, and the device-side compaction of the NMS maxima:
//
//   k10b_minmax        grid (blocks, image): min / max per image
//   k10b_gradients     grid (x, y, image)
//   k10b_likelihood    grid (tile x, tile y, image); the halo is zero-padded at the image's own borders
//   k10b_nms           one thread per scan block: the block's maximum, or "none", into the block's OWN slot
//   k10b_count         one workgroup per 256 slots of one image: how many hold a maximum
//   k10b_offsets       one workgroup: exclusive prefix of the counts in place, cand_offsets[0 .. n_images]
//   k10b_scatter       one workgroup per 256 slots: (u, v, image) at prefix + rank -> ONE list ordered by (image, block id)
//   k10b_refine_score  one wavefront per candidate of the whole batch
//
// Block-id order is nonMaximumSuppression.m's scan order (u outer, v inner), so nothing is sorted and nothing uploaded.
// The host waits twice: for cand_offsets (the refine grid's size), and for the records.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "host_util.h"
#include "ilcc_image_sequence.h"
#include "ilcc_internal.h"
#include "k10_stages.h"

namespace ilcc {

namespace {

constexpr int kSlotChunk = 256;        // slots per compaction workgroup
constexpr uint32_t kMaxBatchImages = 65535;   // the image is gridDim.z / gridDim.y

struct Candidate {   // 1-based (u, v) of an NMS maximum and the image it lies in
  int32_t u, v, image, pad;
};

// one image's share of the plan's device buffer, in bytes from the image's base (every part 256-byte aligned)
struct ImageLayout {
  uint64_t grad, L, slots, end;
};

ImageLayout image_layout(int32_t w, int32_t h) {
  const uint64_t npx = (uint64_t)w * h, nblk = (uint64_t)nms_blocks(w) * nms_blocks(h);
  ImageLayout l;
  l.grad = 0;
  l.L = align256(npx * sizeof(short2));
  l.slots = l.L + align256(npx * sizeof(float));
  l.end = l.slots + align256(nblk * sizeof(int2));
  return l;
}

uint64_t chunks_per_image(int32_t w, int32_t h) { return ((uint64_t)nms_blocks(w) * nms_blocks(h) + kSlotChunk - 1) / kSlotChunk; }

// the batch as the kernels see it
struct BatchArgs {
  const uint8_t* images;
  uint64_t image_pitch;
  uint8_t* scratch;        // image m's share at m * per_image
  uint64_t per_image;
  ImageLayout lay;
  uint32_t* mm;            // [n_images][2]
  uint32_t* counts;        // [n_images * cpi + 1]: per chunk, then its exclusive prefix
  uint32_t* cand_offsets;  // [n_images + 1]
  Candidate* cand;
  Record* rec;
  int32_t w, h, stride, nbx, nby;
  uint32_t n_images, cpi, total;

  __device__ const uint8_t* image(uint32_t m) const { return images + (uint64_t)m * image_pitch; }
  __device__ short2* grad(uint32_t m) const { return (short2*)(scratch + (uint64_t)m * per_image + lay.grad); }
  __device__ float* L(uint32_t m) const { return (float*)(scratch + (uint64_t)m * per_image + lay.L); }
  __device__ int2* slots(uint32_t m) const { return (int2*)(scratch + (uint64_t)m * per_image + lay.slots); }
};

__global__ void k10b_minmax(BatchArgs a) { minmax_body(a.image(blockIdx.y), a.w, a.h, a.stride, a.mm + 2 * blockIdx.y, blockIdx.x, gridDim.x); }

__global__ void k10b_gradients(BatchArgs a) {
  gradients_body(a.image(blockIdx.z), a.w, a.h, a.stride, a.grad(blockIdx.z), blockIdx.x * blockDim.x + threadIdx.x,
                 blockIdx.y * blockDim.y + threadIdx.y);
}

__global__ __launch_bounds__(kTile* kTile) void k10b_likelihood(BatchArgs a) {
  __shared__ float tile[kTileIn][kTileIn];
  likelihood_body(a.image(blockIdx.z), a.w, a.h, a.stride, a.mm + 2 * blockIdx.z, a.L(blockIdx.z), blockIdx.x, blockIdx.y, tile);
}

// slot b of image m: the 1-based (u, v) of block b's maximum; u = 0: none (a maximum has u >= 9)
__global__ __launch_bounds__(kSlotChunk) void k10b_nms(BatchArgs a) {
  const int b = blockIdx.x * kSlotChunk + threadIdx.x;
  if (b >= a.nbx * a.nby) return;
  int maxi, maxj;
  const bool hit = nms_block(a.L(blockIdx.y), a.w, a.h, a.nby, b, maxi, maxj);
  a.slots(blockIdx.y)[b] = hit ? make_int2(maxi, maxj) : make_int2(0, 0);
}

// chunk c of image m = slots [256 c, 256 c + 256) of that image; workgroup m * cpi + c
__device__ __forceinline__ bool slot_of(const BatchArgs& a, int2& s) {
  const uint32_t m = blockIdx.x / a.cpi, b = (blockIdx.x % a.cpi) * kSlotChunk + threadIdx.x;
  const bool in = b < (uint32_t)(a.nbx * a.nby);
  if (in) s = a.slots(m)[b];
  return in && s.x != 0;
}

__global__ __launch_bounds__(kSlotChunk) void k10b_count(BatchArgs a) {
  __shared__ uint32_t sc[17];
  int2 s = make_int2(0, 0);
  uint32_t total;
  (void)block_rank(slot_of(a, s), sc, total);
  if (threadIdx.x == 0) a.counts[blockIdx.x] = total;
}

// one workgroup.  Tile by tile: inclusive scan inside each wavefront, the wavefronts' totals through LDS, a carry between tiles.
__global__ __launch_bounds__(kSlotChunk) void k10b_offsets(BatchArgs a) {
  __shared__ uint32_t wave_total[kSlotChunk / ILCC_WAVE];
  const uint32_t n_chunks = a.n_images * a.cpi;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n_chunks; base += kSlotChunk) {   // uniform trip count
    const uint32_t k = base + threadIdx.x;
    const uint32_t v = k < n_chunks ? a.counts[k] : 0u;
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
    for (int w = 0; w < kSlotChunk / ILCC_WAVE; ++w) {
      const uint32_t t = wave_total[w];
      if (w < wave_id()) before += t;
      tile += t;
    }
    if (k < n_chunks) a.counts[k] = carry + before + incl - v;
    carry += tile;
    __syncthreads();   // wave_total is rewritten by the next tile
  }
  if (threadIdx.x == 0) a.counts[n_chunks] = carry;
  __syncthreads();   // the prefix, written by this workgroup, is read back below by other threads of it
  for (uint32_t m = threadIdx.x; m <= a.n_images; m += kSlotChunk) a.cand_offsets[m] = a.counts[m * a.cpi];
}

__global__ __launch_bounds__(kSlotChunk) void k10b_scatter(BatchArgs a) {
  __shared__ uint32_t sc[17];
  int2 s = make_int2(0, 0);
  uint32_t total;
  const bool keep = slot_of(a, s);
  const uint32_t rank = block_rank(keep, sc, total);
  if (keep) {
    Candidate c;
    c.u = s.x;
    c.v = s.y;
    c.image = (int32_t)(blockIdx.x / a.cpi);
    c.pad = 0;
    a.cand[a.counts[blockIdx.x] + rank] = c;   // below the batch's total, which is at most one per slot
  }
}

__global__ __launch_bounds__(kWave) void k10b_refine_score(BatchArgs a) {
  const uint32_t k = blockIdx.x;
  if (k >= a.total) return;
  const Candidate c = a.cand[k];
  RefineImage im;
  im.img = a.image(c.image);
  im.grad = a.grad(c.image);
  im.mm = a.mm + 2 * c.image;
  im.w = a.w;
  im.h = a.h;
  im.stride = a.stride;
  refine_score_body(im, c.u, c.v, &a.rec[k]);
}

}  // namespace
}  // namespace ilcc

using namespace ilcc;

// One device allocation for everything but the records: [per-image shares][mm][mm's initial words][counts][cand_offsets][cand].
// The records have a device and a page-locked buffer of their own, which grow; the counts come back through h_offsets.
struct ilcc_image_corner_plan {
  uint32_t max_images = 0;
  int32_t max_w = 0, max_h = 0;
  int device = 0;
  uint8_t* d_buf = nullptr;
  uint64_t per_image = 0, at_mm = 0, at_mm_init = 0, at_counts = 0, at_offsets = 0, at_cand = 0;
  uint32_t* h_offsets = nullptr;   // page-locked, max_images + 1
  Record* d_rec = nullptr;
  Record* h_rec = nullptr;         // page-locked
  uint64_t rec_cap = 0;
  uint32_t launches = 0, allocations = 0;
  uint32_t last_n = 0;
};

namespace {

void plan_free(ilcc_image_corner_plan* p) {
  if (!p) return;
  if (p->d_buf) (void)hipFree(p->d_buf);
  if (p->d_rec) (void)hipFree(p->d_rec);
  if (p->h_rec) (void)hipHostFree(p->h_rec);
  if (p->h_offsets) (void)hipHostFree(p->h_offsets);
  delete p;
}

int32_t grow_records(ilcc_image_corner_plan* p, uint64_t need) {
  if (need <= p->rec_cap) return ILCC_OK;
  uint64_t cap = p->rec_cap ? p->rec_cap : 1024;
  while (cap < need) cap *= 2;
  if (p->d_rec) (void)hipFree(p->d_rec);
  if (p->h_rec) (void)hipHostFree(p->h_rec);
  p->d_rec = p->h_rec = nullptr;
  p->rec_cap = 0;
  hipError_t e = hipMalloc((void**)&p->d_rec, cap * sizeof(Record));
  if (e == hipSuccess) e = hipHostMalloc((void**)&p->h_rec, cap * sizeof(Record), hipHostMallocDefault);
  if (e != hipSuccess) return k10_hip_fail("record buffers", e);
  p->allocations += 2;
  p->rec_cap = cap;
  return ILCC_OK;
}

}  // namespace

extern "C" {

uint64_t ilcc_image_corner_scratch_bytes(int32_t width, int32_t height) {
  if (width < kMinSide || height < kMinSide || width > 65536 || height > 65536) return 0;
  const uint64_t nblk = (uint64_t)nms_blocks(width) * nms_blocks(height);
  return image_layout(width, height).end + align256(nblk * sizeof(Candidate));
}

ilcc_image_corner_plan* ilcc_image_corner_plan_create(uint32_t max_images, int32_t max_width, int32_t max_height) {
  if (max_images == 0 || max_images > kMaxBatchImages || max_width < kMinSide || max_height < kMinSide || max_width > 65536 ||
      max_height > 65536) {
    set_global_error("ilcc_image_corner_plan_create: 1 .. 65535 images of 34 .. 65536 px a side");
    return nullptr;
  }
  ilcc_image_corner_plan* p = new (std::nothrow) ilcc_image_corner_plan;
  if (!p) {
    set_global_error("ilcc_image_corner_plan_create: out of memory");
    return nullptr;
  }
  if (hipGetDevice(&p->device) != hipSuccess || p->device < 0 || p->device >= 16) {
    delete p;
    (void)no_device();
    return nullptr;
  }
  p->max_images = max_images;
  p->max_w = max_width;
  p->max_h = max_height;
  const uint64_t n = max_images, nblk = (uint64_t)nms_blocks(max_width) * nms_blocks(max_height);
  p->per_image = image_layout(max_width, max_height).end;
  p->at_mm = n * p->per_image;
  p->at_mm_init = p->at_mm + align256(n * 8);
  p->at_counts = p->at_mm_init + align256(n * 8);
  p->at_offsets = p->at_counts + align256((n * chunks_per_image(max_width, max_height) + 1) * 4);
  p->at_cand = p->at_offsets + align256((n + 1) * 4);
  const uint64_t total = p->at_cand + align256(std::max<uint64_t>(n * nblk, 1) * sizeof(Candidate));
  hipError_t e = hipMalloc((void**)&p->d_buf, total);
  if (e == hipSuccess) {
    ++p->allocations;
    e = hipHostMalloc((void**)&p->h_offsets, (n + 1) * 4, hipHostMallocDefault);
  }
  if (e == hipSuccess) {
    ++p->allocations;
    // the words every call starts an image's min / max from; h_offsets carries them up once
    std::vector<uint32_t> init(2 * n);
    for (uint64_t m = 0; m < n; ++m) {
      init[2 * m] = 0xFFFFFFFFu;
      init[2 * m + 1] = 0u;
    }
    e = hipMemcpy(p->d_buf + p->at_mm_init, init.data(), 8 * n, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    (void)k10_hip_fail("plan buffers", e);
    plan_free(p);
    return nullptr;
  }
  if (grow_records(p, std::max<uint64_t>(1024, 256 * n)) != ILCC_OK) {
    plan_free(p);
    return nullptr;
  }
  return p;
}

void ilcc_image_corner_plan_destroy(ilcc_image_corner_plan* plan) { plan_free(plan); }

uint32_t ilcc_image_corner_plan_launches(const ilcc_image_corner_plan* plan) { return plan ? plan->launches : 0; }

uint32_t ilcc_image_corner_plan_allocations(const ilcc_image_corner_plan* plan) { return plan ? plan->allocations : 0; }

int32_t ilcc_image_corners_batch_device(const void* d_images, uint64_t image_pitch, uint32_t n_images, int32_t width, int32_t height,
                                        int32_t stride, ilcc_image_corner* corners, int32_t capacity, int32_t* n_corners,
                                        ilcc_image_corner_plan* plan, void* hip_stream) {
  if (!plan || capacity < 0) return fail(ILCC_BAD_ARGUMENT, "ilcc_image_corners_batch_device: null plan or negative capacity");
  if (n_images > plan->max_images)
    return fail(ILCC_BAD_ARGUMENT, "ilcc_image_corners_batch_device: " + std::to_string(n_images) + " images, the plan holds " +
                                       std::to_string(plan->max_images));
  if (n_images == 0) {
    plan->launches = 0;
    plan->last_n = 0;
    return ILCC_OK;
  }
  if (!d_images || !n_corners || (capacity > 0 && !corners))
    return fail(ILCC_BAD_ARGUMENT, "ilcc_image_corners_batch_device: null images, output or counts");
  if (width < kMinSide || height < kMinSide)
    return fail(ILCC_BAD_ARGUMENT, "ilcc_image_corners_batch_device: image " + std::to_string(width) + " x " + std::to_string(height) +
                                       " is smaller than " + std::to_string(kMinSide) + " px a side (2 x 12 + 2 x 5)");
  if (width > plan->max_w || height > plan->max_h)
    return fail(ILCC_BAD_ARGUMENT, "ilcc_image_corners_batch_device: image " + std::to_string(width) + " x " + std::to_string(height) +
                                       " is larger than the plan's " + std::to_string(plan->max_w) + " x " + std::to_string(plan->max_h));
  if (stride < width)
    return fail(ILCC_BAD_ARGUMENT, "ilcc_image_corners_batch_device: stride " + std::to_string(stride) + " below width " + std::to_string(width));
  if (image_pitch < (uint64_t)stride * (uint64_t)height)
    return fail(ILCC_BAD_ARGUMENT, "ilcc_image_corners_batch_device: image_pitch " + std::to_string(image_pitch) + " below stride * height");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev != plan->device) return fail(ILCC_BAD_ARGUMENT, "ilcc_image_corners_batch_device: the plan belongs to another device");
  const int32_t taps = ensure_taps(dev);
  if (taps != ILCC_OK) return taps;

  ilcc_image_corner_plan* p = plan;
  hipStream_t s = (hipStream_t)hip_stream;
  BatchArgs a;
  a.images = (const uint8_t*)d_images;
  a.image_pitch = image_pitch;
  a.scratch = p->d_buf;
  a.lay = image_layout(width, height);
  a.per_image = a.lay.end;   // packed by this call's size: within the plan's share, which is sized for the largest
  a.mm = (uint32_t*)(p->d_buf + p->at_mm);
  a.counts = (uint32_t*)(p->d_buf + p->at_counts);
  a.cand_offsets = (uint32_t*)(p->d_buf + p->at_offsets);
  a.cand = (Candidate*)(p->d_buf + p->at_cand);
  a.rec = p->d_rec;
  a.w = width;
  a.h = height;
  a.stride = stride;
  a.nbx = nms_blocks(width);
  a.nby = nms_blocks(height);
  a.n_images = n_images;
  a.cpi = (uint32_t)chunks_per_image(width, height);
  a.total = 0;
  const uint64_t npx = (uint64_t)width * height, nblk = (uint64_t)a.nbx * a.nby;
  uint32_t launches = 0;
  hipError_t e = hipMemcpyAsync(a.mm, p->d_buf + p->at_mm_init, 8ull * n_images, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) {
    const unsigned blocks = (unsigned)std::min<uint64_t>((npx + 255) / 256, 1024);
    hipLaunchKernelGGL(k10b_minmax, dim3(blocks, n_images), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k10b_gradients, dim3((width + 31) / 32, (height + 7) / 8, n_images), dim3(32, 8), 0, s, a);
    hipLaunchKernelGGL(k10b_likelihood, dim3((width + kTile - 1) / kTile, (height + kTile - 1) / kTile, n_images), dim3(kTile, kTile), 0, s, a);
    launches += 3;
    if (nblk) {
      hipLaunchKernelGGL(k10b_nms, dim3(a.cpi, n_images), dim3(kSlotChunk), 0, s, a);
      hipLaunchKernelGGL(k10b_count, dim3(a.cpi * n_images), dim3(kSlotChunk), 0, s, a);
      launches += 2;
    }
    hipLaunchKernelGGL(k10b_offsets, dim3(1), dim3(kSlotChunk), 0, s, a);   // with no scan block: every offset 0
    ++launches;
    if (nblk) {
      hipLaunchKernelGGL(k10b_scatter, dim3(a.cpi * n_images), dim3(kSlotChunk), 0, s, a);
      ++launches;
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(p->h_offsets, a.cand_offsets, 4ull * (n_images + 1), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);   // wait 1: the counts
  if (e != hipSuccess) return k10_hip_fail("launch", e);
  const uint32_t total = p->h_offsets[n_images];
  if ((uint64_t)total > (uint64_t)n_images * nblk) return fail(ILCC_HIP_ERROR, "k10b: more candidates than scan blocks");   // cannot happen
  if (total) {
    const int32_t st = grow_records(p, total);
    if (st != ILCC_OK) return st;
    a.rec = p->d_rec;
    a.total = total;
    hipLaunchKernelGGL(k10b_refine_score, dim3(total), dim3(kWave), 0, s, a);
    ++launches;
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(p->h_rec, p->d_rec, sizeof(Record) * (uint64_t)total, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // wait 2: the records
    if (e != hipSuccess) return k10_hip_fail("refine", e);
  }
  p->launches = launches;
  p->last_n = n_images;
  int32_t st = ILCC_OK;
  for (uint32_t m = 0; m < n_images; ++m) {
    const uint32_t at = p->h_offsets[m], nc = p->h_offsets[m + 1] - at;
    const int32_t cnt = finish_corners(p->h_rec + at, nc, capacity ? corners + (uint64_t)m * capacity : nullptr, capacity);
    n_corners[m] = cnt;
    if (cnt > capacity) {
      set_global_error("ilcc_image_corners_batch_device: image " + std::to_string(m) + ": " + std::to_string(cnt) + " corners exceed capacity " +
                       std::to_string(capacity));
      st = ILCC_CAPACITY;
    }
  }
  return st;
}

int32_t ilcc_image_corner_plan_candidates(ilcc_image_corner_plan* plan, int32_t* candidates, uint32_t capacity, uint32_t* offsets) {
  if (!plan || !offsets || (capacity && !candidates)) return fail(ILCC_BAD_ARGUMENT, "ilcc_image_corner_plan_candidates: null argument");
  const uint32_t n = plan->last_n, total = n ? plan->h_offsets[n] : 0;
  offsets[0] = 0;
  for (uint32_t m = 0; m < n; ++m) offsets[m + 1] = plan->h_offsets[m + 1];
  if (total > capacity) return fail(ILCC_CAPACITY, "ilcc_image_corner_plan_candidates: " + std::to_string(total) + " candidates exceed the capacity");
  if (!total) return ILCC_OK;
  std::vector<Candidate> c(total);
  const hipError_t e = hipMemcpy(c.data(), plan->d_buf + plan->at_cand, sizeof(Candidate) * (uint64_t)total, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return k10_hip_fail("candidates", e);
  for (uint32_t k = 0; k < total; ++k) {
    candidates[3 * k] = c[k].image;
    candidates[3 * k + 1] = c[k].u;
    candidates[3 * k + 2] = c[k].v;
  }
  return ILCC_OK;
}

}  // extern "C"
