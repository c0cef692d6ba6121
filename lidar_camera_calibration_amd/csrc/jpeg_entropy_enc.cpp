// Host half of include/ilcc_jpeg_write.h: the info of a file to write, and the baseline Huffman encoder (ITU-T T.81 B,
// F.1.2, Annex K tables) from quantised coefficients in the decoder's layout to the bytes of the file, as libjpeg writes
// them.  Plain C++17: no HIP, no allocation, nothing written past `cap`; it builds alone with csrc/jpeg_entropy.cpp
// (tests/jpeg_write_host_check.cpp links only these two, under sanitizers).
// Little-endian or big-endian host alike: every multi-byte field is written byte by byte.
#include <cstdio>
#include <cstring>

#include "ilcc_hip.h"
#include "ilcc_jpeg_write.h"
#include "ilcc_jpeg_write_sequence.h"
#include "jpeg_annex_k.h"
#include "jpeg_entropy.h"

namespace {

using ilcc::jpeg_refuse;
using namespace ilcc::annex_k;

// T.81 Annex K.1, natural order: luminance, chrominance
constexpr uint8_t kStdQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// symbol -> code and its length
struct Codes {
  uint16_t code[256];
  uint8_t length[256];

  void define(const uint8_t* counts, const uint8_t* symbols) {
    std::memset(length, 0, sizeof(length));
    uint32_t next = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < counts[len - 1]; ++i, ++k, ++next) {
        code[symbols[k]] = (uint16_t)next;
        length[symbols[k]] = (uint8_t)len;
      }
      next <<= 1;
    }
  }
};

// bytes into [out, out + cap): past the end they are counted, not stored
struct Writer {
  uint8_t* out;
  uint64_t cap, at = 0;
  uint64_t acc = 0;   // the low `nacc` bits wait for their byte boundary
  int nacc = 0;

  void byte(uint32_t v) {
    if (at < cap) out[at] = (uint8_t)v;
    ++at;
  }
  void u16(uint32_t v) {
    byte(v >> 8);
    byte(v & 255u);
  }
  void marker(uint32_t m) {
    byte(0xFF);
    byte(m);
  }
  void bits(uint32_t value, int length) {   // length <= 32, value < 2^length
    acc = (acc << length) | value;
    nacc += length;
    while (nacc >= 8) {
      nacc -= 8;
      const uint32_t b = (uint32_t)(acc >> nacc) & 255u;
      byte(b);
      if (b == 255u) byte(0);
    }
  }
  void pad() {   // 1-bits up to the byte boundary
    if (nacc) bits((1u << (8 - nacc)) - 1u, 8 - nacc);
  }
};

int bit_length(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }

// what beyond the layout the writer needs of an info: table indices 0 / 1, 8-bit quantisation entries, a 16-bit interval
const char* unwritable(const ilcc_jpeg_info& I) {
  if (!ilcc::jpeg_laid_out(I)) return "the info's block counts and offsets are not ilcc_jpeg_layout's";
  if (I.restart_interval < 0 || I.restart_interval > 65535) return "restart interval outside 0 .. 65535";
  for (int c = 0; c < I.n_components; ++c) {
    const ilcc_jpeg_component& C = I.comp[c];
    if (C.quant_index > 1 || C.dc_table < 0 || C.dc_table > 1 || C.ac_table < 0 || C.ac_table > 1) return "table index outside 0 .. 1";
    for (int k = 0; k < 64; ++k)
      if (I.quant[C.quant_index][k] < 1 || I.quant[C.quant_index][k] > 255) return "quantisation entry outside 1 .. 255";
  }
  return nullptr;
}

uint64_t total_blocks(const ilcc_jpeg_info& I) { return I.coef_count / 64u; }

uint64_t total_mcus(const ilcc_jpeg_info& I) {
  return (uint64_t)(I.comp[0].blocks_w / I.comp[0].h) * (uint64_t)(I.comp[0].blocks_h / I.comp[0].v);
}

void write_headers(Writer& w, const ilcc_jpeg_info& I) {
  w.marker(0xD8);
  w.marker(0xE0);
  w.u16(16);
  for (int k = 0; k < 5; ++k) w.byte((uint8_t)"JFIF"[k]);   // with its terminating 0
  w.u16(0x0101);   // version 1.01
  w.byte(0);       // no units: the densities are an aspect ratio
  w.u16(1);
  w.u16(1);
  w.u16(0);        // no thumbnail
  bool sent[2] = {false, false};
  for (int c = 0; c < I.n_components; ++c) {
    const int t = I.comp[c].quant_index;
    if (sent[t]) continue;
    sent[t] = true;
    w.marker(0xDB);
    w.u16(67);
    w.byte((uint32_t)t);
    for (int k = 0; k < 64; ++k) w.byte(I.quant[t][kZigzag[k]]);
  }
  w.marker(0xC0);
  w.u16(8 + 3 * (uint32_t)I.n_components);
  w.byte(8);
  w.u16((uint32_t)I.height);
  w.u16((uint32_t)I.width);
  w.byte((uint32_t)I.n_components);
  for (int c = 0; c < I.n_components; ++c) {
    w.byte((uint32_t)c + 1);
    w.byte((uint32_t)((I.comp[c].h << 4) | I.comp[c].v));
    w.byte((uint32_t)I.comp[c].quant_index);
  }
  bool dc_sent[2] = {false, false}, ac_sent[2] = {false, false};
  for (int c = 0; c < I.n_components; ++c) {
    const int td = I.comp[c].dc_table, ta = I.comp[c].ac_table;
    if (!dc_sent[td]) {
      dc_sent[td] = true;
      w.marker(0xC4);
      w.u16(2 + 1 + 16 + 12);
      w.byte((uint32_t)td);
      for (int k = 0; k < 16; ++k) w.byte(kDcCounts[td][k]);
      for (int k = 0; k < 12; ++k) w.byte(kDcSymbols[k]);
    }
    if (!ac_sent[ta]) {
      ac_sent[ta] = true;
      w.marker(0xC4);
      w.u16(2 + 1 + 16 + 162);
      w.byte(0x10u | (uint32_t)ta);
      for (int k = 0; k < 16; ++k) w.byte(kAcCounts[ta][k]);
      for (int k = 0; k < 162; ++k) w.byte(kAcSymbols[ta][k]);
    }
  }
  if (I.restart_interval) {
    w.marker(0xDD);
    w.u16(4);
    w.u16((uint32_t)I.restart_interval);
  }
  w.marker(0xDA);
  w.u16(6 + 2 * (uint32_t)I.n_components);
  w.byte((uint32_t)I.n_components);
  for (int c = 0; c < I.n_components; ++c) {
    w.byte((uint32_t)c + 1);
    w.byte((uint32_t)((I.comp[c].dc_table << 4) | I.comp[c].ac_table));
  }
  w.byte(0);     // spectral selection 0 .. 63, no successive approximation
  w.byte(63);
  w.byte(0);
}

}  // namespace

extern "C" {

int32_t ilcc_jpeg_write_info(int32_t width, int32_t height, int32_t n_components, int32_t sampling_h, int32_t sampling_v, int32_t quality,
                             int32_t restart_interval, ilcc_jpeg_info* out) {
  if (!out) return jpeg_refuse("ilcc_jpeg_write_info: null argument");
  if (n_components != 1 && n_components != 3) return jpeg_refuse("1 or 3 components only");
  if (restart_interval < 0 || restart_interval > 65535) return jpeg_refuse("restart interval outside 0 .. 65535");
  ilcc_jpeg_info I;
  std::memset(&I, 0, sizeof(I));
  I.width = width;
  I.height = height;
  I.n_components = n_components;
  I.restart_interval = restart_interval;
  for (int c = 0; c < n_components; ++c) {
    I.comp[c].h = c == 0 && n_components == 3 ? sampling_h : 1;
    I.comp[c].v = c == 0 && n_components == 3 ? sampling_v : 1;
    I.comp[c].quant_index = I.comp[c].dc_table = I.comp[c].ac_table = c ? 1 : 0;
  }
  const int32_t q = quality < 1 ? 1 : quality > 100 ? 100 : quality;
  const int32_t scale = q < 50 ? 5000 / q : 200 - 2 * q;
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) {
      const int32_t v = (kStdQuant[t][k] * scale + 50) / 100;
      I.quant[t][k] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
  const int32_t st = ilcc_jpeg_layout(&I);   // refuses the size and the sampling
  if (st != ILCC_OK) return st;
  *out = I;
  return ILCC_OK;
}

uint64_t ilcc_jpeg_file_bound(const ilcc_jpeg_info* info) {
  if (!info || !ilcc::jpeg_laid_out(*info)) return 0;
  // SOI, APP0, 2 DQT, SOF0, 4 DHT, DRI, SOS, EOI; every scan byte stuffed; a pad byte (stuffed) and a marker per interval
  const uint64_t headers = 2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + 6 + 14 + 2;
  const uint64_t scan = 2 * ((total_blocks(*info) * kWorstBlockBits + 7) / 8);
  const uint64_t restarts = info->restart_interval > 0 ? total_mcus(*info) / (uint64_t)info->restart_interval : 0;
  return headers + scan + 4 * restarts + 2;
}

int32_t ilcc_jpeg_write_headers(const ilcc_jpeg_info* info, uint8_t* out, uint64_t cap, uint64_t* bytes) {
  if (!info || !bytes || (!out && cap)) return jpeg_refuse("ilcc_jpeg_write_headers: null argument");
  *bytes = 0;
  if (const char* why = unwritable(*info)) return jpeg_refuse("ilcc_jpeg_write_headers", why);
  Writer w{out, cap};
  write_headers(w, *info);
  if (w.at > cap) {
    jpeg_refuse("output buffer smaller than the headers");
    return ILCC_CAPACITY;
  }
  *bytes = w.at;
  return ILCC_OK;
}

int32_t ilcc_jpeg_entropy_encode(const ilcc_jpeg_info* info, const int16_t* coef, uint8_t* out, uint64_t cap, uint64_t* bytes) {
  if (!info || !coef || !bytes || (!out && cap)) return jpeg_refuse("ilcc_jpeg_entropy_encode: null argument");
  *bytes = 0;
  const ilcc_jpeg_info& I = *info;
  if (const char* why = unwritable(I)) return jpeg_refuse("ilcc_jpeg_entropy_encode", why);
  Codes dc[2], ac[2];
  for (int t = 0; t < 2; ++t) {
    dc[t].define(kDcCounts[t], kDcSymbols);
    ac[t].define(kAcCounts[t], kAcSymbols[t]);
  }
  Writer w{out, cap};
  write_headers(w, I);

  const int nc = I.n_components;
  const int32_t mcus_w = I.comp[0].blocks_w / I.comp[0].h;
  const uint64_t total = total_mcus(I);
  const uint64_t interval = (uint64_t)I.restart_interval;
  int32_t pred[3] = {0, 0, 0};
  uint64_t to_go = interval;
  uint32_t next_rst = 0;
  for (uint64_t mcu = 0; mcu < total; ++mcu) {
    if (interval) {
      if (to_go == 0) {
        w.pad();
        w.marker(0xD0u + next_rst);
        next_rst = (next_rst + 1) & 7u;
        pred[0] = pred[1] = pred[2] = 0;
        to_go = interval;
      }
      --to_go;
    }
    if (w.at > cap) break;   // the rest could only be counted
    const int32_t my = (int32_t)(mcu / (uint64_t)mcus_w), mx = (int32_t)(mcu % (uint64_t)mcus_w);
    for (int c = 0; c < nc; ++c) {
      const ilcc_jpeg_component& C = I.comp[c];
      const Codes& D = dc[C.dc_table];
      const Codes& A = ac[C.ac_table];
      for (int dy = 0; dy < C.v; ++dy)
        for (int dx = 0; dx < C.h; ++dx) {
          const int16_t* block = coef + C.coef_offset + ((uint64_t)(my * C.v + dy) * (uint64_t)C.blocks_w + (uint64_t)(mx * C.h + dx)) * 64u;
          const int32_t diff = (int32_t)block[0] - pred[c];
          pred[c] = block[0];
          int n = bit_length((uint32_t)(diff < 0 ? -diff : diff));
          if (n > kMaxDcBits) return jpeg_refuse("coefficient libjpeg refuses", "DC difference outside 11 bits");
          w.bits(D.code[n], D.length[n]);
          if (n) w.bits((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u), n);   // T.81 F.1.2.1: negative values one less
          int run = 0;
          for (int k = 1; k < 64; ++k) {
            const int32_t v = block[kZigzag[k]];
            if (v == 0) {
              ++run;
              continue;
            }
            for (; run > 15; run -= 16) w.bits(A.code[0xF0], A.length[0xF0]);
            n = bit_length((uint32_t)(v < 0 ? -v : v));
            if (n > kMaxAcBits) return jpeg_refuse("coefficient libjpeg refuses", "AC value outside 10 bits");
            const int rs = (run << 4) | n;
            w.bits(((uint32_t)A.code[rs] << n) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u)), A.length[rs] + n);
            run = 0;
          }
          if (run) w.bits(A.code[0], A.length[0]);   // EOB
        }
    }
  }
  w.pad();
  w.marker(0xD9);
  if (w.at > cap) {
    jpeg_refuse("output buffer smaller than the file");
    return ILCC_CAPACITY;
  }
  *bytes = w.at;
  return ILCC_OK;
}

}  // extern "C"
