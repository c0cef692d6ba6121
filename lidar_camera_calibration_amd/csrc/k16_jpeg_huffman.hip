// K16 -- the Huffman scans of a batch of JPEG frames of one geometry decoded on the device (include/ilcc_jpeg_huffman.h states the
// method, the launches and the rules; this file follows that text).  Input: the unstuffed scans, the tables and the segment rows
// ilcc_jpeg_scan_prepare makes; output: the coefficients exactly as ilcc_jpeg_entropy_decode leaves them, K13b's input.
//
// k16_clear   zeroes coefficients (16 bytes a lane), statuses and counters.
// k16_decode  one workgroup per segment; subsequences of S bits, chunks of kThreads subsequences, everything between threads in LDS
//             behind __syncthreads.  A chunk's bytes (256 * S / 8, 64 KB at S = 2048) are staged in dynamic LDS once, as aligned
//             dwords where the source allows, and every pass of the chunk reads its bits from there: a symbol costs two LDS dword
//             reads where a global load would cost its whole latency, which nothing hides at one workgroup an image.
//             Every row a workgroup reads from device memory is checked against the arrays' and the image's sizes before it is
//             used, and every store is to a block index below the segment's block count of an MCU below the image's MCU count:
//             garbage in any input cannot move a store out of image m's coef_count int16.
// k16_dc      one workgroup per (segment, component): DC differences -> DC values.
#include <hip/hip_runtime.h>

#include <string>

#include "host_util.h"
#include "ilcc_hip.h"
#include "ilcc_jpeg_huffman.h"
#include "jpeg_entropy.h"

namespace ilcc {

constexpr int kThreads = 256;             // of k16_decode and k16_dc; subsequences in a chunk

__constant__ uint8_t kZigzagDev[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffmanComponent {
  uint64_t coef_offset;
  uint32_t blocks_w;
  uint32_t h, v;
};

struct HuffmanArgs {
  const uint8_t* scans;
  uint64_t scans_bytes;
  const ilcc_jpeg_huffman_tables* tables;
  const ilcc_jpeg_huffman_segment* segments;
  const ilcc_jpeg_huffman_image* images;
  int16_t* coef;
  uint64_t coef_pitch;
  uint64_t coef_count;
  uint32_t* status;
  ilcc_jpeg_huffman_counters* counters;
  uint32_t n_images, n_segments;
  uint32_t sub_bits;         // S
  uint32_t n_components;
  uint32_t units;            // blocks in an MCU
  uint32_t mcus_w, mcus;     // MCUs in a row, in the image
  uint32_t luma_units;       // the MCU's first luma_units blocks are component 0's, h0 in a row; then one of each other component
  uint32_t luma_h;
  HuffmanComponent comp[3];
};

__device__ inline uint32_t unit_component(const HuffmanArgs& a, uint32_t unit) { return unit < a.luma_units ? 0u : unit - a.luma_units + 1u; }

__global__ __launch_bounds__(256) void k16_clear(HuffmanArgs a) {
  const uint64_t m = blockIdx.y;
  const uint64_t at = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 8u;   // coef_pitch and d_coef are multiples of 16 bytes
  int16_t* image = a.coef + m * a.coef_pitch;
  if (at + 8u <= a.coef_count) {
    *reinterpret_cast<uint4*>(image + at) = make_uint4(0, 0, 0, 0);
  } else {
    for (uint64_t k = at; k < a.coef_count; ++k) image[k] = 0;   // coef_count is a multiple of 64: never taken, kept for the bound
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.status[m] = 0;
    a.counters[m] = ilcc_jpeg_huffman_counters{0, 0, 0, 0};
  }
}

// A decoder state: the bit position in the segment, and (block inside the MCU) << 8 | coefficient index (0: a DC code is next).
struct State {
  uint32_t pos, where;
};

struct Segment {
  const uint8_t* bytes;
  uint32_t n_bytes, n_bits;
  uint32_t blocks;           // the segment's block count
  uint32_t first_mcu;
  // the chunk in LDS: words[0] holds the segment's bytes staged_from .. staged_from + 3 (in memory order), zeros outside the segment
  const uint32_t* words;
  int32_t staged_from;       // byte offset in the segment, -3 .. : the source's dword boundary at or in front of the chunk
};

constexpr uint32_t kStagedSlack = 32;   // bytes of LDS behind a chunk's own: the dword in front, a symbol's look-ahead, the second dword of a read

// 32 bits from bit `pos` on, zeros behind the segment's end; pos lies inside the staged chunk
__device__ inline uint32_t peek32(const Segment& s, uint32_t pos) {
  const uint32_t b = (uint32_t)((int32_t)(pos >> 3) - s.staged_from);
  const uint64_t two = ((uint64_t)__builtin_bswap32(s.words[b >> 2]) << 32) | __builtin_bswap32(s.words[(b >> 2) + 1]);
  return (uint32_t)((two << ((b & 3u) * 8u + (pos & 7u))) >> 32);
}

// Stages the segment's bytes [first, first + count + look-ahead) for the passes of one chunk; every thread of the workgroup calls it.
__device__ inline void stage_chunk(Segment* s, uint32_t* lds, uint32_t first, uint32_t count) {
  const uint32_t mis = (uint32_t)((uintptr_t)(s->bytes + first) & 3u);
  s->words = lds;
  s->staged_from = (int32_t)first - (int32_t)mis;
  const uint32_t n_words = (mis + count + 8u + 3u) / 4u + 1u;              // <= (256 * S / 8 + kStagedSlack) / 4
  const uint8_t* from = s->bytes + s->staged_from;                          // dword aligned; may lie up to 3 bytes in front of the segment
  for (uint32_t w = threadIdx.x; w < n_words; w += blockDim.x) {
    const int64_t at = (int64_t)s->staged_from + 4 * (int64_t)w;            // byte offset in the segment
    uint32_t v = 0;
    if (at >= 0 && at + 4 <= (int64_t)s->n_bytes) {
      v = *reinterpret_cast<const uint32_t*>(from + 4 * (size_t)w);
    } else {
      for (int j = 0; j < 4; ++j)
        if (at + j >= 0 && at + j < (int64_t)s->n_bytes) v |= (uint32_t)s->bytes[at + j] << (8 * j);
    }
    lds[w] = v;
  }
}

// the code at the head of `bits` (16 valid bits at the top of a 32-bit window): -> its length, 0: in no table
__device__ inline uint32_t huffman_symbol(const ilcc_jpeg_huffman_table& t, uint32_t window, uint32_t* sym) {
  const uint32_t code16 = window >> 16;
  const uint32_t e = t.look[code16 >> 7];
  if (e) {
    *sym = e & 255u;
    return (e >> 8) <= 9u ? e >> 8 : 0u;   // a length no table of the host's holds: garbage, "in no table"
  }
  for (uint32_t len = 10; len <= 16; ++len) {
    const int32_t code = (int32_t)(code16 >> (16 - len));
    if (code <= t.maxcode[len]) {
      *sym = t.values[(uint32_t)(t.first[len] + code) & 255u];
      return len;
    }
  }
  return 0;
}

// Decodes from `st` to the first symbol boundary at or behind bit `end`; -> the blocks completed.
// WRITE false: a guess or a count: nothing is an error (the rules are in the header).
// WRITE true: from an exact state, `block` being the segment-order index of the block `st` is in: stores coefficients, stops at the
// segment's block count or at the first thing the host decoder refuses, whose bit goes into *fault.
template <bool WRITE>
__device__ inline uint32_t decode_span(const HuffmanArgs& a, const ilcc_jpeg_huffman_tables& T, const Segment& s, State* st, uint32_t end,
                                       uint32_t block, int16_t* image, uint32_t* fault) {
  uint32_t pos = st->pos, unit = st->where >> 8, k = st->where & 255u, done = 0;
  int16_t* dst = nullptr;
  bool placed = false;
  while (pos < end) {
    if (WRITE) {
      if (block >= s.blocks) break;
      if (!placed) {   // the block's address: (MCU, block in MCU) -> (component, bx, by)
        const uint32_t mcu = s.first_mcu + block / a.units, u = block % a.units;   // < a.mcus: checked with the row
        const uint32_t c = unit_component(a, u);
        const HuffmanComponent& K = c == 0 ? a.comp[0] : c == 1 ? a.comp[1] : a.comp[2];
        const uint32_t dx = c ? 0u : u % a.luma_h, dy = c ? 0u : u / a.luma_h;
        const uint32_t bx = (mcu % a.mcus_w) * K.h + dx, by = (mcu / a.mcus_w) * K.v + dy;
        dst = image + K.coef_offset + ((uint64_t)by * K.blocks_w + bx) * 64u;
        placed = true;
      }
    }
    const uint32_t c = unit_component(a, unit);
    const uint32_t window = peek32(s, pos);
    const uint32_t left = s.n_bits - pos;
    uint32_t sym = 0;
    const uint32_t len = huffman_symbol(k == 0 ? T.dc[c] : T.ac[c], window, &sym);
    bool close = false;
    if (len == 0) {
      if (WRITE) {
        *fault |= left < 16 ? ILCC_JPEG_HUFFMAN_ENDS_EARLY : ILCC_JPEG_HUFFMAN_NO_CODE;
        break;
      }
      pos += 1;
      continue;
    }
    if (len > left) {
      if (WRITE) *fault |= ILCC_JPEG_HUFFMAN_ENDS_EARLY;
      pos = s.n_bits;
      break;
    }
    uint32_t size, at = k, next = k + 1;   // the coefficient the symbol's extra bits hold, and the one behind it
    if (k == 0) {
      size = sym;
      if (size > 15) {
        if (WRITE) {
          *fault |= ILCC_JPEG_HUFFMAN_DC_CATEGORY;
          break;
        }
        size = 0;
      }
    } else {
      const uint32_t run = sym >> 4;
      size = sym & 15u;
      if (size == 0) {
        if (run != 15) {
          close = true;              // EOB
        } else if (k + 16 > 64) {
          if (WRITE) {
            *fault |= ILCC_JPEG_HUFFMAN_RUN_PAST_63;
            break;
          }
          close = true;
        } else {
          next = k + 16;             // ZRL
        }
      } else if (k + run > 63) {
        if (WRITE) {
          *fault |= ILCC_JPEG_HUFFMAN_RUN_PAST_63;
          break;
        }
        size = 0;
        close = true;
      } else {
        at = k + run;
        next = at + 1;
      }
    }
    if (len + size > left) {
      if (WRITE) *fault |= ILCC_JPEG_HUFFMAN_ENDS_EARLY;
      pos = s.n_bits;
      break;
    }
    pos += len + size;
    if (WRITE && size) {   // T.81 F.2.2.1 EXTEND of the `size` bits behind the code
      const int32_t raw = (int32_t)((window << len) >> (32 - size));
      const int32_t v = raw >= (1 << (size - 1)) ? raw : raw - (1 << size) + 1;
      dst[kZigzagDev[at]] = (int16_t)v;   // at <= 63; size <= 15: |v| <= 32767
    }
    k = next;
    if (k >= 64) close = true;
    if (close) {
      k = 0;
      unit = unit + 1 == a.units ? 0 : unit + 1;
      done += 1;
      if (WRITE) {
        block += 1;
        placed = false;
      }
    }
  }
  st->pos = pos;
  st->where = (unit << 8) | k;
  return done;
}

__global__ __launch_bounds__(kThreads) void k16_decode(HuffmanArgs a) {
  __shared__ ilcc_jpeg_huffman_tables T;
  __shared__ State exits[kThreads];
  __shared__ uint32_t wave_sums[kThreads / 64];
  extern __shared__ uint32_t staged[];   // kThreads * S / 8 + kStagedSlack bytes

  const uint32_t m = blockIdx.y, t = threadIdx.x;
  const ilcc_jpeg_huffman_image im = a.images[m];
  if (blockIdx.x >= im.n_segments) return;                      // the whole workgroup
  uint32_t bad = 0;
  if (im.scan_offset > a.scans_bytes || im.scan_bytes > a.scans_bytes - im.scan_offset || im.first_segment > a.n_segments ||
      im.n_segments > a.n_segments - im.first_segment)
    bad = 1;
  ilcc_jpeg_huffman_segment row{0, 0, 0, 0};
  if (!bad) {
    row = a.segments[im.first_segment + blockIdx.x];
    if (row.byte_offset > im.scan_bytes || row.byte_count > im.scan_bytes - row.byte_offset || row.byte_count >= (1u << 28) ||
        row.first_mcu > a.mcus || row.mcu_count > a.mcus - row.first_mcu)
      bad = 1;
  }
  if (bad) {                                                     // uniform: the rows are the same for every thread
    if (t == 0) atomicOr(&a.status[m], ILCC_JPEG_HUFFMAN_BAD_ROWS);
    return;
  }
  {   // the image's tables, 16 bytes a lane
    const uint4* from = reinterpret_cast<const uint4*>(a.tables + m);
    uint4* to = reinterpret_cast<uint4*>(&T);
    for (uint32_t k = t; k < sizeof(T) / 16; k += kThreads) to[k] = from[k];
  }
  Segment s;
  s.bytes = a.scans + im.scan_offset + row.byte_offset;
  s.n_bytes = row.byte_count;
  s.n_bits = row.byte_count * 8u;
  s.blocks = row.mcu_count * a.units;                           // <= 2^26 MCUs of at most 6 blocks
  s.first_mcu = row.first_mcu;
  int16_t* image = a.coef + (uint64_t)m * a.coef_pitch;
  const uint32_t S = a.sub_bits;
  const uint32_t n_sub = (s.n_bits + S - 1) / S;
  __syncthreads();

  State entry{0, 0};           // exact, of the chunk's first subsequence
  uint32_t first_block = 0;    // of the chunk, in the segment's order
  uint32_t fault = 0, chunks = 0, rounds_sum = 0, rounds_max = 0;
  for (uint32_t base = 0; base < n_sub && first_block < s.blocks; base += kThreads) {
    const uint32_t n = n_sub - base < (uint32_t)kThreads ? n_sub - base : (uint32_t)kThreads;
    const bool live = t < n;
    stage_chunk(&s, staged, base * (S / 8u), n * (S / 8u));
    __syncthreads();
    const uint32_t end = (base + t + 1) * S < s.n_bits ? (base + t + 1) * S : s.n_bits;   // (base + t + 1) * S < 2^31 + 2^19 for live threads
    // cold pass
    State from = t == 0 ? entry : State{(base + t) * S, 0};
    State out = from;
    uint32_t done = 0;
    if (live) done = decode_span<false>(a, T, s, &out, end, 0, nullptr, nullptr);
    if (live) exits[t] = out;
    __syncthreads();
    // rounds: at most n - 1, subsequence i is exact after round i
    uint32_t rounds = 0;
    for (uint32_t r = 1; r < n; ++r) {
      State left = from;
      if (live && t > 0) left = exits[t - 1];
      __syncthreads();
      int changed = 0;
      if (live && t > 0 && (left.pos != from.pos || left.where != from.where)) {
        from = left;
        State now = from;
        done = decode_span<false>(a, T, s, &now, end, 0, nullptr, nullptr);
        changed = now.pos != out.pos || now.where != out.where;
        out = now;
        exits[t] = out;
      }
      rounds += 1;
      if (!__syncthreads_or(changed)) break;
    }
    // count and place: an exclusive prefix sum of the blocks each subsequence completes
    uint32_t scan = live ? done : 0;
    const uint32_t lane = t & 63u, wave = t >> 6;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(scan, d, 64);
      if (lane >= d) scan += up;
    }
    if (lane == 63) wave_sums[wave] = scan;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < kThreads / 64; ++w) {
      if (w < wave) before += wave_sums[w];
      total += wave_sums[w];
    }
    const uint32_t my_first = first_block + before + scan - (live ? done : 0);
    // write: once more from the exact state
    if (live) {
      State st = from;
      decode_span<true>(a, T, s, &st, end, my_first, image, &fault);
    }
    entry = exits[n - 1];
    first_block += total;      // a guess never counts past 2^28 * 8 bits: no overflow
    chunks += 1;
    rounds_sum += rounds;
    rounds_max = rounds > rounds_max ? rounds : rounds_max;
    __syncthreads();           // exits and wave_sums are written again by the next chunk
  }
  if (first_block < s.blocks) fault |= ILCC_JPEG_HUFFMAN_ENDS_EARLY;   // the bits ended before the blocks did
  if (fault) atomicOr(&a.status[m], fault);
  if (t == 0) {
    ilcc_jpeg_huffman_counters* c = a.counters + m;
    atomicAdd(&c->subsequences, n_sub);
    atomicAdd(&c->chunks, chunks);
    atomicAdd(&c->rounds, rounds_sum);
    atomicMax(&c->max_rounds, rounds_max);
  }
}

// DC differences -> DC values for component blockIdx.y of segment blockIdx.x of image blockIdx.z
__global__ __launch_bounds__(kThreads) void k16_dc(HuffmanArgs a) {
  __shared__ int32_t wave_sums[kThreads / 64];
  const uint32_t m = blockIdx.z, c = blockIdx.y, t = threadIdx.x;
  const ilcc_jpeg_huffman_image im = a.images[m];
  if (blockIdx.x >= im.n_segments) return;
  if (im.first_segment > a.n_segments || im.n_segments > a.n_segments - im.first_segment) return;   // k16_decode has flagged it
  const ilcc_jpeg_huffman_segment row = a.segments[im.first_segment + blockIdx.x];
  if (row.first_mcu > a.mcus || row.mcu_count > a.mcus - row.first_mcu) return;
  const HuffmanComponent K = a.comp[c];
  const uint32_t per_mcu = K.h * K.v;
  const uint32_t n = row.mcu_count * per_mcu;
  int16_t* plane = a.coef + (uint64_t)m * a.coef_pitch + K.coef_offset;
  int32_t carry = 0;
  const uint32_t lane = t & 63u, wave = t >> 6;
  for (uint32_t base = 0; base < n; base += kThreads) {
    const uint32_t j = base + t;
    int16_t* dc = nullptr;
    int32_t v = 0;
    if (j < n) {
      const uint32_t mcu = row.first_mcu + j / per_mcu, u = j % per_mcu;
      const uint32_t bx = (mcu % a.mcus_w) * K.h + u % K.h, by = (mcu / a.mcus_w) * K.v + u / K.h;
      dc = plane + ((uint64_t)by * K.blocks_w + bx) * 64u;
      v = *dc;
    }
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const int32_t up = __shfl_up(v, d, 64);
      if (lane >= d) v += up;
    }
    if (lane == 63) wave_sums[wave] = v;
    __syncthreads();
    int32_t total = 0;
    for (uint32_t w = 0; w < kThreads / 64; ++w) {
      if (w < wave) v += wave_sums[w];
      total += wave_sums[w];
    }
    v += carry;                // |carry| <= 32768 and 256 differences of at most 32767: inside int32
    const int outside = j < n && (v < -32768 || v > 32767);
    if (j < n) *dc = (int16_t)v;
    carry += total;
    if (__syncthreads_or(outside)) {   // also keeps wave_sums until every thread has read it
      if (t == 0) atomicOr(&a.status[m], ILCC_JPEG_HUFFMAN_DC_RANGE);
      return;                  // the image is refused: what is behind stays differences
    }
  }
}

namespace {

int32_t refuse(const std::string& what) {
  set_global_error("ilcc_jpeg_huffman_batch_device: " + what);
  return ILCC_BAD_ARGUMENT;
}

}  // namespace
}  // namespace ilcc

extern "C" uint64_t ilcc_jpeg_huffman_scratch_bytes(uint32_t n_images) { return (uint64_t)n_images * sizeof(ilcc_jpeg_huffman_counters); }

extern "C" int32_t ilcc_jpeg_huffman_batch_device(const ilcc_jpeg_huffman_job* job) {
  using namespace ilcc;
  if (!job) return refuse("null job");
  const ilcc_jpeg_huffman_job& J = *job;
  if (!J.layout || !J.d_scans || !J.d_tables || !J.d_segments || !J.d_images || !J.d_coef || !J.d_status || !J.d_scratch)
    return refuse("null pointer");
  if (!jpeg_laid_out(*J.layout)) return refuse("the layout's block counts and offsets are not ilcc_jpeg_layout's");
  const ilcc_jpeg_info& I = *J.layout;
  if (J.n_images > 65535u) return refuse("more than 65535 images");
  if (J.coef_pitch < I.coef_count || (J.coef_pitch & 7u)) return refuse("coef_pitch must hold coef_count and be a multiple of 8");
  if ((uintptr_t)J.d_coef & 15u) return refuse("d_coef must be 16-byte aligned");
  if ((uintptr_t)J.d_tables & 15u) return refuse("d_tables must be 16-byte aligned");
  if ((uintptr_t)J.d_segments & 15u) return refuse("d_segments must be 16-byte aligned");
  if ((uintptr_t)J.d_images & 7u) return refuse("d_images must be 8-byte aligned");
  if ((uintptr_t)J.d_status & 3u) return refuse("d_status must be 4-byte aligned");
  if ((uintptr_t)J.d_scratch & 15u) return refuse("d_scratch must be 16-byte aligned");
  if (J.scratch_bytes < ilcc_jpeg_huffman_scratch_bytes(J.n_images)) return refuse("scratch_bytes is less than ilcc_jpeg_huffman_scratch_bytes");
  const uint32_t S = J.subsequence_bits ? J.subsequence_bits : ILCC_JPEG_HUFFMAN_DEFAULT_BITS;
  if (S != 256 && S != 512 && S != 1024 && S != 2048) return refuse("subsequence_bits must be 0, 256, 512, 1024 or 2048");
  if (J.n_images == 0) return ILCC_OK;
  if (J.max_segments == 0 || J.max_segments > J.n_segments) return refuse("max_segments must be 1 .. n_segments");

  HuffmanArgs a{};
  a.scans = J.d_scans;
  a.scans_bytes = J.scans_bytes;
  a.tables = J.d_tables;
  a.segments = J.d_segments;
  a.images = J.d_images;
  a.coef = J.d_coef;
  a.coef_pitch = J.coef_pitch;
  a.coef_count = I.coef_count;
  a.status = J.d_status;
  a.counters = (ilcc_jpeg_huffman_counters*)J.d_scratch;
  a.n_images = J.n_images;
  a.n_segments = J.n_segments;
  a.sub_bits = S;
  a.n_components = (uint32_t)I.n_components;
  a.mcus_w = (uint32_t)(I.comp[0].blocks_w / I.comp[0].h);
  a.mcus = a.mcus_w * (uint32_t)(I.comp[0].blocks_h / I.comp[0].v);
  uint32_t units = 0;
  for (int c = 0; c < I.n_components; ++c) {   // the MCU's blocks in the order the scan holds them
    HuffmanComponent& K = a.comp[c];
    K.coef_offset = I.comp[c].coef_offset;
    K.blocks_w = (uint32_t)I.comp[c].blocks_w;
    K.h = (uint32_t)I.comp[c].h;
    K.v = (uint32_t)I.comp[c].v;
    units += K.h * K.v;
  }
  a.units = units;   // jpeg_laid_out: 1, 3, 4 or 6; chroma is 1 x 1
  a.luma_units = a.comp[0].h * a.comp[0].v;
  a.luma_h = a.comp[0].h;
  hipStream_t s = (hipStream_t)J.hip_stream;
  const uint64_t groups = (I.coef_count / 8u + 255u) / 256u;
  if (groups > 0x7FFFFFFFull) return refuse("coef_count too large for one launch");
  const uint32_t chunk_lds = (uint32_t)kThreads * S / 8u + kStagedSlack;
  // 64 KB + 32 at S = 2048 is above the default limit.  The limit is always set to the value of the LARGEST accepted S, whatever this
  // call's S: every caller writes the same value, so calls on several host threads (or devices) cannot lower it under one another.
  constexpr int kLargestChunkLds = kThreads * 2048 / 8 + (int)kStagedSlack;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k16_decode), hipFuncAttributeMaxDynamicSharedMemorySize, kLargestChunkLds);
  if (e != hipSuccess) {
    set_global_error(std::string("k16: dynamic LDS of k16_decode: ") + hipGetErrorString(e));
    return ILCC_HIP_ERROR;
  }
  hipLaunchKernelGGL(k16_clear, dim3((uint32_t)groups, J.n_images), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k16_decode, dim3(J.max_segments, J.n_images), dim3(kThreads), chunk_lds, s, a);
  hipLaunchKernelGGL(k16_dc, dim3(J.max_segments, (uint32_t)I.n_components, J.n_images), dim3(kThreads), 0, s, a);
  e = hipGetLastError();
  if (e != hipSuccess) {
    set_global_error(std::string("k16 launch: ") + hipGetErrorString(e));
    return ILCC_HIP_ERROR;
  }
  return ILCC_OK;
}
