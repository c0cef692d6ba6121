// K17 -- the Huffman scans of a batch of images encoded on the GPU (include/ilcc_jpeg_write_sequence.h, which states the contract
// and the eight launches; tests/jpeg_huffman_enc_ref.py restates the steps in numpy).  The bytes are the ones the scan loop of
// csrc/jpeg_entropy_enc.cpp writes on one host core; the tables are that file's (csrc/jpeg_annex_k.h).
//
// Encoding, unlike decoding, needs no synchronisation: a block's bits follow from its 64 coefficients and the DC of the block
// before it in its component, which index arithmetic finds.  So the work is lengths (k17_count), prefix sums (k17_layout,
// k17_place_unstuffed), and a scatter of codes to known bit offsets (k17_pack).  Byte stuffing makes the output's length depend on
// its own bytes, hence the second half: the 0xFF bytes are counted per 4096 bytes (k17_count_ff), prefixed (k17_place), and every
// byte moves to its index plus the 0xFF bytes before it (k17_stuff).
//
// A thread of k17_count and k17_pack owns one block: it loads the block's 128 bytes as eight 16-byte loads into registers and
// walks them in zigzag order with every index a constant (the loop is unrolled), so no coefficient is ever indexed dynamically.
// The Annex-K codes are 2 x (12 + 256) words of code << 8 | length, built at compile time, staged in LDS per workgroup.
// The scans inside a workgroup are Hillis-Steele over 256 values in LDS: eight steps, nothing clever, and the sums they make
// are exact integers whatever the order.
//
// Bounds: k17_pack never writes a word at or past the image's own unstuffed length (rounded up to a word), k17_stuff never a
// byte at or past offset + bytes of the image's row, and k17_place gives an image a row with bytes > 0 only when
// offset + bytes <= out_cap.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "host_util.h"
#include "ilcc_hip.h"
#include "ilcc_jpeg_write_sequence.h"
#include "jpeg_annex_k.h"
#include "jpeg_entropy.h"

namespace ilcc {
namespace k17 {

constexpr int kThreads = 256;
constexpr uint32_t kTile = 256;              // blocks whose bit counts one workgroup prefixes
constexpr uint32_t kChunk = 4096;            // unstuffed bytes one workgroup counts and stuffs; the alignment of an image there
constexpr uint32_t kGranule = kChunk / kThreads;   // 16 bytes a thread
constexpr uint32_t kFlagShift = 24;          // a tile's sum is below 2^20: its refusal bits ride above it
constexpr uint32_t kUnpacked = 0x100u;       // internal: the image has no room in the unstuffed buffer
constexpr uint32_t kRangeBits = ILCC_JPEG_ENCODE_DC_RANGE | ILCC_JPEG_ENCODE_AC_RANGE;
static_assert(kGranule == 16, "a thread of k17_count_ff and k17_stuff reads one uint4");

// code << 8 | length by symbol; length 0: the symbol has no code (never looked up for an accepted coefficient)
struct Codes {
  uint32_t dc[2][12];
  uint32_t ac[2][256];
  uint8_t zigzag[64];
};

constexpr Codes make_codes() {
  Codes c{};
  for (int t = 0; t < 2; ++t) {
    uint32_t next = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < annex_k::kDcCounts[t][len - 1]; ++i, ++k, ++next) c.dc[t][annex_k::kDcSymbols[k]] = (next << 8) | (uint32_t)len;
      next <<= 1;
    }
    next = 0;
    k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < annex_k::kAcCounts[t][len - 1]; ++i, ++k, ++next) c.ac[t][annex_k::kAcSymbols[t][k]] = (next << 8) | (uint32_t)len;
      next <<= 1;
    }
  }
  for (int k = 0; k < 64; ++k) c.zigzag[k] = annex_k::kZigzag[k];
  return c;
}

__device__ const Codes kCodes = make_codes();

// what the kernels need of the layout
struct Geometry {
  uint32_t n_blocks, n_tiles, n_segments;
  uint32_t segment_blocks;       // blocks of every segment but the last
  uint32_t interval;             // MCUs of a segment (the whole scan without restart markers)
  uint32_t mcus_w, mcu_blocks;   // MCUs a row, blocks an MCU
  uint32_t h0, v0;               // luma's sampling: the first h0 v0 blocks of an MCU are luma's, then one Cb, one Cr
  // no arrays here: a kernel argument indexed by a component that is only known at run time would be copied to scratch
  uint32_t luma_blocks_w, chroma_blocks_w;
  uint32_t dc_tables, ac_tables;   // bit c: component c's Huffman table, 0 luma's or 1 chroma's
  uint64_t luma_offset, cb_offset, chroma_stride;   // of the components' first blocks, int16: Cr's is cb_offset + chroma_stride
  uint64_t coef_pitch;
};

struct Scratch {
  uint32_t* blk;        // [n][n_blocks]      a block's bit offset inside its tile
  uint32_t* tile;       // [n][n_tiles + 1]   k17_count: the tile's bits | flags << 24; k17_layout: the exclusive prefix, [n_tiles] the sum
  uint32_t* seg;        // [n][n_segments + 1] a segment's byte offset in the image's unstuffed scan; [n_segments] the scan's length
  uint32_t* img;        // [n][2]             unstuffed bytes (0: refused), flags
  uint64_t* u_off;      // [n + 1]            the image's offset in the unstuffed buffer; [n] the end of the last image that has room
  uint16_t* ff_local;   // [ubuf_cap / 16]    0xFF bytes of the chunk in front of the granule
  uint32_t* ff_chunk;   // [ubuf_cap / 4096 + 1] k17_count_ff: the chunk's 0xFF bytes; k17_place: the exclusive prefix (it may wrap: only differences are used)
  uint8_t* ubuf;
  uint64_t ubuf_cap;    // a multiple of 4096
};

template <class T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* lds, T* total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
#pragma unroll
  for (int d = 1; d < kThreads; d <<= 1) {
    const T x = t >= d ? lds[t - d] : T(0);
    __syncthreads();
    lds[t] += x;
    __syncthreads();
  }
  const T inclusive = lds[t];
  *total = lds[kThreads - 1];
  __syncthreads();
  return inclusive - v;
}

__device__ __forceinline__ void stage_codes(uint32_t (&dc)[2][12], uint32_t (&ac)[2][256]) {
  const int t = threadIdx.x;
  (&ac[0][0])[t] = (&kCodes.ac[0][0])[t];
  (&ac[0][0])[t + 256] = (&kCodes.ac[0][0])[t + 256];
  if (t < 24) (&dc[0][0])[t] = (&kCodes.dc[0][0])[t];
  __syncthreads();
}

// where block `s` (scan order) of an image lies, and which component it belongs to
struct BlockAt {
  uint64_t offset;     // of its coefficients, int16
  uint32_t component;
  bool first_of_component;   // in its MCU
  uint32_t mcu;
};

__device__ __forceinline__ uint64_t block_offset(const Geometry& g, uint32_t mcu, uint32_t c, uint32_t dy, uint32_t dx) {
  const uint32_t my = mcu / g.mcus_w, mx = mcu - my * g.mcus_w;
  const uint32_t h = c == 0 ? g.h0 : 1u, v = c == 0 ? g.v0 : 1u;
  const uint32_t bw = c == 0 ? g.luma_blocks_w : g.chroma_blocks_w;
  const uint64_t off = c == 0 ? g.luma_offset : g.cb_offset + (uint64_t)(c - 1) * g.chroma_stride;
  return off + ((uint64_t)(my * v + dy) * bw + (uint64_t)mx * h + dx) * 64u;
}

__device__ __forceinline__ BlockAt block_at(const Geometry& g, uint32_t s) {
  BlockAt b;
  b.mcu = s / g.mcu_blocks;
  const uint32_t r = s - b.mcu * g.mcu_blocks, luma = g.h0 * g.v0;
  if (r < luma) {
    b.component = 0;
    b.first_of_component = r == 0;
    b.offset = block_offset(g, b.mcu, 0, r / g.h0, r % g.h0);
  } else {
    b.component = 1 + (r - luma);
    b.first_of_component = true;
    b.offset = block_offset(g, b.mcu, b.component, 0, 0);
  }
  return b;
}

// the DC of the block before `s` in its component, 0 at a segment's start
__device__ __forceinline__ int32_t predictor(const Geometry& g, const int16_t* coef, uint32_t s, const BlockAt& b) {
  if (!b.first_of_component) {   // luma's second to fourth block of an MCU: the block before it in the scan
    const uint32_t r = s - b.mcu * g.mcu_blocks - 1;
    return coef[block_offset(g, b.mcu, 0, r / g.h0, r % g.h0)];
  }
  if (b.mcu % g.interval == 0) return 0;
  return b.component == 0 ? coef[block_offset(g, b.mcu - 1, 0, g.v0 - 1, g.h0 - 1)] : coef[block_offset(g, b.mcu - 1, b.component, 0, 0)];
}

__device__ __forceinline__ void load_block(const int16_t* block, uint32_t (&w)[32]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint4 q = reinterpret_cast<const uint4*>(block)[k];
    w[4 * k] = q.x;
    w[4 * k + 1] = q.y;
    w[4 * k + 2] = q.z;
    w[4 * k + 3] = q.w;
  }
}

// The codes of one block in order: put(bits, length) for each, length 1 .. 26.  Returns the refusal bits; a refused value is
// clamped to its limit so that every table index stays inside its table (the image takes no bytes anyway).
template <class Put>
__device__ __forceinline__ uint32_t walk_block(const uint32_t (&w)[32], int32_t pred, const uint32_t* dc, const uint32_t* ac, Put&& put) {
  uint32_t flags = 0;
  const int32_t diff = (int32_t)(int16_t)(w[0] & 0xFFFFu) - pred;
  uint32_t mag = (uint32_t)(diff < 0 ? -diff : diff);
  uint32_t n = mag ? 32u - (uint32_t)__clz(mag) : 0u;
  if (n > (uint32_t)annex_k::kMaxDcBits) {
    flags |= ILCC_JPEG_ENCODE_DC_RANGE;
    n = annex_k::kMaxDcBits;
  }
  {
    const uint32_t e = dc[n];
    put(((e >> 8) << n) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u)), (e & 255u) + n);   // T.81 F.1.2.1: negative values one less
  }
  uint32_t run = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    const int nat = kCodes.zigzag[k];
    const int32_t v = (int32_t)(int16_t)((w[nat >> 1] >> (16 * (nat & 1))) & 0xFFFFu);
    if (v == 0) {
      ++run;
      continue;
    }
    for (; run > 15; run -= 16) put(ac[0xF0] >> 8, ac[0xF0] & 255u);
    mag = (uint32_t)(v < 0 ? -v : v);
    n = 32u - (uint32_t)__clz(mag);
    if (n > (uint32_t)annex_k::kMaxAcBits) {
      flags |= ILCC_JPEG_ENCODE_AC_RANGE;
      n = annex_k::kMaxAcBits;
    }
    const uint32_t e = ac[(run << 4) | n];
    put(((e >> 8) << n) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u)), (e & 255u) + n);
    run = 0;
  }
  if (run) put(ac[0] >> 8, ac[0] & 255u);   // EOB
  return flags;
}

__global__ __launch_bounds__(kThreads) void k17_clear(uint4* ubuf, uint64_t n16) {
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n16; i += stride) ubuf[i] = make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(kThreads) void k17_count(Geometry g, const int16_t* coef, Scratch sc) {
  __shared__ uint32_t s_dc[2][12], s_ac[2][256], s_scan[kThreads], s_flags;
  if (threadIdx.x == 0) s_flags = 0;
  stage_codes(s_dc, s_ac);
  const uint32_t m = blockIdx.y, s = blockIdx.x * kTile + threadIdx.x;
  uint32_t bits = 0;
  if (s < g.n_blocks) {
    const int16_t* image = coef + (uint64_t)m * g.coef_pitch;
    const BlockAt b = block_at(g, s);
    uint32_t w[32];
    load_block(image + b.offset, w);
    const uint32_t td = (g.dc_tables >> b.component) & 1u, ta = (g.ac_tables >> b.component) & 1u;
    const uint32_t flags = walk_block(w, predictor(g, image, s, b), s_dc[td], s_ac[ta], [&](uint32_t, uint32_t length) { bits += length; });
    if (flags) atomicOr(&s_flags, flags);
  }
  uint32_t total;
  const uint32_t before = block_exclusive_scan(bits, s_scan, &total);   // its barriers order s_flags too
  if (s < g.n_blocks) sc.blk[(uint64_t)m * g.n_blocks + s] = before;
  if (threadIdx.x == 0) sc.tile[(uint64_t)m * (g.n_tiles + 1) + blockIdx.x] = total | (s_flags << kFlagShift);
}

// bit offset of block x in its image's scan with the segments laid end to end, x <= n_blocks
__device__ __forceinline__ uint32_t bits_before(const Geometry& g, const uint32_t* tile, const uint32_t* blk, uint32_t x) {
  return x >= g.n_blocks ? tile[g.n_tiles] : tile[x / kTile] + blk[x];
}

__global__ __launch_bounds__(kThreads) void k17_layout(Geometry g, Scratch sc) {
  __shared__ uint32_t s_scan[kThreads], s_flags;
  const uint32_t m = blockIdx.x, t = threadIdx.x;
  uint32_t* tile = sc.tile + (uint64_t)m * (g.n_tiles + 1);
  const uint32_t* blk = sc.blk + (uint64_t)m * g.n_blocks;
  uint32_t* seg = sc.seg + (uint64_t)m * (g.n_segments + 1);
  if (t == 0) s_flags = 0;
  __syncthreads();
  uint32_t carry = 0, flags = 0;
  for (uint32_t base = 0; base < g.n_tiles; base += kThreads) {   // bounded by the layout
    const uint32_t i = base + t;
    const uint32_t v = i < g.n_tiles ? tile[i] : 0u;
    flags |= v >> kFlagShift;
    uint32_t total;
    const uint32_t before = block_exclusive_scan(v & ((1u << kFlagShift) - 1u), s_scan, &total);
    if (i < g.n_tiles) tile[i] = carry + before;
    carry += total;
  }
  if (t == 0) tile[g.n_tiles] = carry;
  if (flags) atomicOr(&s_flags, flags);
  __syncthreads();   // the prefix is visible to the whole workgroup, and so are the flags
  flags = s_flags;
  if (flags) {       // refused: no bytes, and nothing behind reads its segments
    if (t == 0) {
      sc.img[2 * m] = 0;
      sc.img[2 * m + 1] = flags;
    }
    return;
  }
  carry = 0;
  for (uint32_t base = 0; base < g.n_segments; base += kThreads) {
    const uint32_t k = base + t;
    uint32_t bytes = 0;
    if (k < g.n_segments) {
      const uint32_t first = k * g.segment_blocks, end = min(first + g.segment_blocks, g.n_blocks);
      bytes = (bits_before(g, tile, blk, end) - bits_before(g, tile, blk, first) + 7u) / 8u + (k + 1 < g.n_segments ? 2u : 0u);
    }
    uint32_t total;
    const uint32_t before = block_exclusive_scan(bytes, s_scan, &total);
    if (k < g.n_segments) seg[k] = carry + before;
    carry += total;
  }
  if (t == 0) {
    seg[g.n_segments] = carry;
    sc.img[2 * m] = carry;
    sc.img[2 * m + 1] = 0;
  }
}

__device__ __forceinline__ uint64_t up_chunk(uint64_t bytes) { return (bytes + (kChunk - 1)) & ~(uint64_t)(kChunk - 1); }

// An image has room when its end (rounded up to a chunk) is inside the buffer.  The offsets never decrease, so once one image has
// none, none behind it has: each decides for itself.
__global__ __launch_bounds__(kThreads) void k17_place_unstuffed(uint32_t n, Scratch sc) {
  __shared__ uint64_t s_scan[kThreads];
  const uint32_t t = threadIdx.x;
  uint64_t carry = 0;
  for (uint32_t base = 0; base < n; base += kThreads) {   // n <= 65535
    const uint32_t m = base + t;
    const uint64_t a = m < n ? up_chunk(sc.img[2 * m]) : 0;
    uint64_t total;
    const uint64_t off = carry + block_exclusive_scan(a, s_scan, &total);
    if (m < n) {
      const bool fits = off + a <= sc.ubuf_cap;
      sc.u_off[m] = fits ? off : ~0ull;
      if (!fits) {
        sc.img[2 * m + 1] |= kUnpacked;
        if (off <= sc.ubuf_cap) sc.u_off[n] = off;   // the first one without room: the images in front of it end here
      }
    }
    carry += total;
  }
  if (t == 0 && carry <= sc.ubuf_cap) sc.u_off[n] = carry;   // all of them have room
}

struct BitWriter {
  uint32_t* words;
  uint32_t at, limit;     // word index; words at or past `limit` are not the image's
  uint64_t acc;           // the top `n` bits wait for their word
  uint32_t n;
  bool shared;            // the word being filled holds bits of another block in front of this one's

  __device__ __forceinline__ void flush(uint32_t word, bool whole) {
    if (at < limit) {
      const uint32_t v = __builtin_bswap32(word);   // the stream is big-endian
      if (whole) words[at] = v;
      else atomicOr(&words[at], v);
    }
    ++at;
  }
  __device__ __forceinline__ void put(uint32_t value, uint32_t length) {   // length <= 26, value < 2^length
    if (length == 0) return;
    acc |= (uint64_t)value << (64u - n - length);
    n += length;
    if (n >= 32u) {
      flush((uint32_t)(acc >> 32), !shared);
      shared = false;
      acc <<= 32;
      n -= 32u;
    }
  }
  __device__ __forceinline__ void finish() {
    if (n) flush((uint32_t)(acc >> 32), false);
  }
};

__global__ __launch_bounds__(kThreads) void k17_pack(Geometry g, const int16_t* coef, Scratch sc) {
  __shared__ uint32_t s_dc[2][12], s_ac[2][256];
  stage_codes(s_dc, s_ac);
  const uint32_t m = blockIdx.y, s = blockIdx.x * kTile + threadIdx.x;
  if (s >= g.n_blocks || sc.img[2 * m + 1] != 0) return;
  const uint32_t* tile = sc.tile + (uint64_t)m * (g.n_tiles + 1);
  const uint32_t* blk = sc.blk + (uint64_t)m * g.n_blocks;
  const uint32_t* seg = sc.seg + (uint64_t)m * (g.n_segments + 1);
  const uint32_t k = s / g.segment_blocks, first = k * g.segment_blocks;
  const uint32_t start = 8u * seg[k] + (bits_before(g, tile, blk, s) - bits_before(g, tile, blk, first));
  const int16_t* image = coef + (uint64_t)m * g.coef_pitch;
  const BlockAt b = block_at(g, s);
  uint32_t w[32];
  load_block(image + b.offset, w);
  const uint32_t td = (g.dc_tables >> b.component) & 1u, ta = (g.ac_tables >> b.component) & 1u;
  BitWriter bw;
  bw.words = reinterpret_cast<uint32_t*>(sc.ubuf + sc.u_off[m]);
  bw.at = start / 32u;
  bw.limit = (sc.img[2 * m] + 3u) / 4u;
  bw.acc = 0;
  bw.n = start % 32u;
  bw.shared = bw.n != 0;
  uint32_t bits = 0;
  walk_block(w, predictor(g, image, s, b), s_dc[td], s_ac[ta], [&](uint32_t value, uint32_t length) {
    bits += length;
    bw.put(value, length);
  });
  if (s + 1 == min(first + g.segment_blocks, g.n_blocks)) {   // the segment's last block: 1-bits up to the byte boundary
    const uint32_t pad = (0u - (start + bits)) & 7u;
    bw.put((1u << pad) - 1u, pad);
  }
  bw.finish();
}

__device__ __forceinline__ uint32_t count_ff(uint4 q) {
  uint32_t n = 0;
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) n += ((w[i] >> (8 * j)) & 255u) == 255u ? 1u : 0u;
  return n;
}

__global__ __launch_bounds__(kThreads) void k17_count_ff(uint32_t n, Scratch sc) {
  __shared__ uint32_t s_scan[kThreads];
  const uint64_t g0 = (uint64_t)blockIdx.x * kChunk;
  if (g0 >= sc.u_off[n]) return;   // the whole workgroup
  const uint64_t granule = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint32_t ff = count_ff(reinterpret_cast<const uint4*>(sc.ubuf)[granule]);
  uint32_t total;
  sc.ff_local[granule] = (uint16_t)block_exclusive_scan(ff, s_scan, &total);
  if (threadIdx.x == 0) sc.ff_chunk[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void k17_place(uint32_t n, uint64_t out_cap, ilcc_jpeg_encode_row* rows, Scratch sc) {
  __shared__ uint32_t s_scan[kThreads];
  __shared__ uint64_t s_scan64[kThreads];
  const uint32_t t = threadIdx.x;
  const uint64_t chunks = sc.u_off[n] / kChunk;   // <= ubuf_cap / 4096
  uint32_t carry = 0;
  for (uint64_t base = 0; base < chunks; base += kThreads) {
    const uint64_t i = base + t;
    const uint32_t v = i < chunks ? sc.ff_chunk[i] : 0u;
    uint32_t total;
    const uint32_t before = block_exclusive_scan(v, s_scan, &total);
    if (i < chunks) sc.ff_chunk[i] = carry + before;
    carry += total;
  }
  if (t == 0) sc.ff_chunk[chunks] = carry;
  __syncthreads();
  // An image whose end lies past out_cap takes nothing, and since the offsets never decrease and an image's own size is in
  // the next one's offset, every image behind it ends past out_cap too: each decides for itself.
  uint64_t at = 0;
  for (uint32_t base = 0; base < n; base += kThreads) {
    const uint32_t m = base + t;
    uint32_t size = 0, flags = 0;
    if (m < n) {
      size = sc.img[2 * m];
      flags = sc.img[2 * m + 1];
      if (flags == 0) {
        const uint64_t c0 = sc.u_off[m] / kChunk, c1 = c0 + up_chunk(size) / kChunk;
        size += sc.ff_chunk[c1] - sc.ff_chunk[c0];
      }   // without room in the unstuffed buffer: the unstuffed length, a lower bound that already ends past out_cap
    }
    uint64_t total;
    const uint64_t off = at + block_exclusive_scan((uint64_t)((size + 15u) & ~15u), s_scan64, &total);
    if (m < n) {
      const bool fits = off + size <= out_cap;
      ilcc_jpeg_encode_row r;
      r.offset = off;
      r.status = (flags & kRangeBits) | (fits && !(flags & kUnpacked) ? 0u : ILCC_JPEG_ENCODE_CAPACITY);
      r.bytes = r.status ? 0u : size;
      rows[m] = r;
    }
    at += total;
  }
}

__global__ __launch_bounds__(kThreads) void k17_stuff(Geometry g, uint32_t n, uint8_t* out, const ilcc_jpeg_encode_row* rows, Scratch sc) {
  const uint64_t g0 = (uint64_t)blockIdx.x * kChunk;
  if (g0 >= sc.u_off[n]) return;
  // the image this chunk belongs to: the last one that starts at or in front of it (at most 16 steps)
  uint32_t lo = 0, hi = n;   // u_off[lo] <= g0 < u_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (sc.u_off[mid] <= g0) lo = mid;
    else hi = mid;
  }
  const uint32_t m = lo;
  const ilcc_jpeg_encode_row row = rows[m];
  if (row.status != 0) return;
  const uint32_t size = sc.img[2 * m];
  const uint64_t u0 = sc.u_off[m];
  const uint32_t i0 = (uint32_t)(g0 - u0) + threadIdx.x * kGranule;
  if (i0 >= size) return;
  const uint64_t granule = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  uint32_t ff = sc.ff_chunk[blockIdx.x] - sc.ff_chunk[u0 / kChunk] + sc.ff_local[granule];
  const uint32_t* seg = sc.seg + (uint64_t)m * (g.n_segments + 1);
  uint32_t k = 0;
  {   // the segment of byte i0: seg[k] <= i0 < seg[k + 1]
    uint32_t top = g.n_segments;
    while (top - k > 1) {
      const uint32_t mid = (k + top) / 2;
      if (seg[mid] <= i0) k = mid;
      else top = mid;
    }
  }
  uint32_t next = seg[k + 1];
  const uint4 q = reinterpret_cast<const uint4*>(sc.ubuf)[granule];
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
  uint8_t* dst = out + row.offset;
#pragma unroll
  for (uint32_t j = 0; j < kGranule; ++j) {
    const uint32_t i = i0 + j;
    if (i >= size) break;
    while (i >= next && k + 1 < g.n_segments) next = seg[++k + 1];   // a segment is three bytes or more: one step at most
    const uint32_t at = i + ff;
    if (at >= row.bytes) break;   // never: the row's bytes are the sum of what is written here
    uint32_t b = (w[j / 4] >> (8 * (j % 4))) & 255u;
    if (k + 1 < g.n_segments && i + 2 >= next) {   // the hole behind the segment: its RSTn
      dst[at] = i + 2 == next ? 0xFFu : (uint8_t)(0xD0u + (k & 7u));
      continue;
    }
    dst[at] = (uint8_t)b;
    if (b == 255u) {
      if (at + 1 < row.bytes) dst[at + 1] = 0;
      ++ff;
    }
  }
}

namespace {

int32_t refuse(const std::string& what) {
  set_global_error("ilcc_jpeg_huffman_encode_batch_device: " + what);
  return ILCC_BAD_ARGUMENT;
}

// nullptr, or why the layout is not one K17 takes
const char* unusable(const ilcc_jpeg_info& I) {
  if (!jpeg_laid_out(I)) return "the layout's block counts and offsets are not ilcc_jpeg_layout's";
  if (I.restart_interval < 0 || I.restart_interval > 65535) return "restart interval outside 0 .. 65535";
  for (int c = 0; c < I.n_components; ++c) {
    const ilcc_jpeg_component& C = I.comp[c];
    if (C.dc_table < 0 || C.dc_table > 1 || C.ac_table < 0 || C.ac_table > 1) return "table index outside 0 .. 1";
  }
  // every bit offset of an image fits 32 bits: its worst-case blocks and a marker per block
  if ((I.coef_count / 64u) * (annex_k::kWorstBlockBits + 24u) >= (1ull << 32)) return "the layout has too many blocks for 32-bit bit offsets";
  return nullptr;
}

Geometry geometry_of(const ilcc_jpeg_info& I, uint64_t coef_pitch) {
  Geometry g{};
  g.n_blocks = (uint32_t)(I.coef_count / 64u);
  g.n_tiles = (g.n_blocks + kTile - 1) / kTile;
  g.h0 = (uint32_t)I.comp[0].h;
  g.v0 = (uint32_t)I.comp[0].v;
  g.mcus_w = (uint32_t)I.comp[0].blocks_w / g.h0;
  const uint32_t mcus = g.mcus_w * ((uint32_t)I.comp[0].blocks_h / g.v0);
  g.mcu_blocks = I.n_components == 1 ? 1u : g.h0 * g.v0 + 2u;
  g.interval = I.restart_interval > 0 && (uint32_t)I.restart_interval < mcus ? (uint32_t)I.restart_interval : mcus;
  g.n_segments = (mcus + g.interval - 1) / g.interval;
  g.segment_blocks = g.interval * g.mcu_blocks;
  for (int c = 0; c < I.n_components; ++c) {
    g.dc_tables |= (uint32_t)I.comp[c].dc_table << c;
    g.ac_tables |= (uint32_t)I.comp[c].ac_table << c;
  }
  g.luma_blocks_w = (uint32_t)I.comp[0].blocks_w;
  g.luma_offset = I.comp[0].coef_offset;
  if (I.n_components == 3) {   // Cb and Cr share their geometry (ilcc_jpeg_layout: both are sampled 1 x 1)
    g.chroma_blocks_w = (uint32_t)I.comp[1].blocks_w;
    g.cb_offset = I.comp[1].coef_offset;
    g.chroma_stride = I.comp[2].coef_offset - I.comp[1].coef_offset;
  }
  g.coef_pitch = coef_pitch;
  return g;
}

// the parts of the scratch, each on a 256-byte boundary; -> the bytes in all
uint64_t carve(const Geometry& g, uint32_t n, uint64_t out_cap, uint8_t* base, Scratch* sc) {
  uint64_t at = 0;
  auto part = [&](uint64_t bytes) {
    uint8_t* p = base + at;
    at += align256(bytes);
    return p;
  };
  sc->ubuf_cap = ((out_cap + (kChunk - 1)) & ~(uint64_t)(kChunk - 1)) + (uint64_t)kChunk * n;
  sc->blk = (uint32_t*)part(4ull * n * g.n_blocks);
  sc->tile = (uint32_t*)part(4ull * n * (g.n_tiles + 1));
  sc->seg = (uint32_t*)part(4ull * n * (g.n_segments + 1));
  sc->img = (uint32_t*)part(8ull * n);
  sc->u_off = (uint64_t*)part(8ull * (n + 1));
  sc->ff_local = (uint16_t*)part(2ull * (sc->ubuf_cap / kGranule));
  sc->ff_chunk = (uint32_t*)part(4ull * (sc->ubuf_cap / kChunk + 1));
  sc->ubuf = part(sc->ubuf_cap);
  return at;
}

constexpr uint64_t kMaxOutCap = 1ull << 40;

}  // namespace
}  // namespace k17
}  // namespace ilcc

extern "C" uint64_t ilcc_jpeg_huffman_encode_scratch_bytes(const ilcc_jpeg_info* layout, uint32_t n_images, uint64_t out_cap) {
  using namespace ilcc::k17;
  if (!layout || unusable(*layout) || n_images > 65535u || out_cap >= kMaxOutCap) return 0;
  Scratch sc;
  return carve(geometry_of(*layout, 0), n_images, out_cap, nullptr, &sc);
}

extern "C" int32_t ilcc_jpeg_huffman_encode_batch_device(const ilcc_jpeg_huffman_encode_job* job) {
  using namespace ilcc;
  using namespace ilcc::k17;
  if (!job || !job->layout || !job->d_coef || !job->d_out || !job->d_rows || !job->d_scratch) return refuse("null pointer");
  const ilcc_jpeg_huffman_encode_job J = *job;
  if (const char* why = unusable(*J.layout)) return refuse(why);
  const ilcc_jpeg_info& I = *J.layout;
  if (J.n_images > 65535u) return refuse("more than 65535 images");
  if (J.out_cap >= kMaxOutCap) return refuse("out_cap of 2^40 bytes or more");
  if (J.coef_pitch < I.coef_count || (J.coef_pitch & 7u)) return refuse("coef_pitch must hold coef_count and be a multiple of 8");
  if ((uintptr_t)J.d_coef & 15u) return refuse("d_coef must be 16-byte aligned");
  if ((uintptr_t)J.d_out & 15u) return refuse("d_out must be 16-byte aligned");
  if ((uintptr_t)J.d_rows & 7u) return refuse("d_rows must be 8-byte aligned");
  if ((uintptr_t)J.d_scratch & 255u) return refuse("d_scratch must be 256-byte aligned");
  const Geometry g = geometry_of(I, J.coef_pitch);
  Scratch sc;
  if (J.scratch_bytes < carve(g, J.n_images, J.out_cap, (uint8_t*)J.d_scratch, &sc)) return refuse("scratch_bytes is less than ilcc_jpeg_huffman_encode_scratch_bytes");
  if (J.n_images == 0) return ILCC_OK;
  hipStream_t s = (hipStream_t)J.hip_stream;
  const uint32_t n = J.n_images;
  const uint64_t n16 = sc.ubuf_cap / 16u, chunks = sc.ubuf_cap / kChunk;
  if (chunks > 0x7FFFFFFFull) return refuse("out_cap too large for one grid");
  const dim3 block(kThreads);
  const dim3 per_block(g.n_tiles, n), per_chunk((uint32_t)chunks);
  const uint32_t clear_groups = (uint32_t)std::min<uint64_t>((n16 + kThreads - 1) / kThreads, 8192);
  hipLaunchKernelGGL(k17_clear, dim3(clear_groups), block, 0, s, reinterpret_cast<uint4*>(sc.ubuf), n16);
  hipLaunchKernelGGL(k17_count, per_block, block, 0, s, g, J.d_coef, sc);
  hipLaunchKernelGGL(k17_layout, dim3(n), block, 0, s, g, sc);
  hipLaunchKernelGGL(k17_place_unstuffed, dim3(1), block, 0, s, n, sc);
  hipLaunchKernelGGL(k17_pack, per_block, block, 0, s, g, J.d_coef, sc);
  hipLaunchKernelGGL(k17_count_ff, per_chunk, block, 0, s, n, sc);
  hipLaunchKernelGGL(k17_place, dim3(1), block, 0, s, n, J.out_cap, J.d_rows, sc);
  hipLaunchKernelGGL(k17_stuff, per_chunk, block, 0, s, g, n, J.d_out, (const ilcc_jpeg_encode_row*)J.d_rows, sc);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_global_error(std::string("k17 launch: ") + hipGetErrorString(e));
    return ILCC_HIP_ERROR;
  }
  return ILCC_OK;
}
