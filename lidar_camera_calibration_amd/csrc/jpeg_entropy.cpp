// Host half of include/ilcc_jpeg.h: the marker parser and the sequential Huffman decoder (ITU-T T.81 B, F.2),
// from the bytes of a file to quantised, de-zigzagged coefficients.  Plain C++17: no HIP, no allocation, nothing read
// past `bytes`; it builds alone (tests/jpeg_host_check.cpp links only this file, under sanitizers).
// Little-endian or big-endian host alike: every multi-byte field is assembled from bytes.
#include <cstdio>
#include <cstring>

#include "ilcc_hip.h"
#include "ilcc_jpeg.h"
#include "jpeg_entropy.h"
#include "jpeg_tables.h"

namespace ilcc {

void (*jpeg_error_sink)(const char*) = nullptr;

namespace {
thread_local char g_jpeg_error[160] = "";
}

const char* jpeg_last_error() { return g_jpeg_error; }

}  // namespace ilcc

namespace ilcc {

int32_t jpeg_refuse(const char* cause, const char* detail) {
  char* text = g_jpeg_error;
  if (detail) std::snprintf(text, sizeof(g_jpeg_error), "jpeg: %s (%s)", cause, detail);
  else std::snprintf(text, sizeof(g_jpeg_error), "jpeg: %s", cause);
  if (jpeg_error_sink) jpeg_error_sink(text);
  return ILCC_BAD_ARGUMENT;
}

}  // namespace ilcc

namespace {

int32_t refuse(const char* cause, const char* detail = nullptr) { return ilcc::jpeg_refuse(cause, detail); }

// natural (row-major) index of the k-th coefficient in zigzag order
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLookBits = ilcc::kJpegLookBits;
using Huffman = ilcc::JpegHuffman;   // csrc/jpeg_tables.h: shared with csrc/jpeg_scan_prepare.cpp
using Tables = ilcc::JpegTables;

struct Reader {
  const uint8_t* m;
  uint64_t n, at;
  bool u8(uint32_t* v) {
    if (at >= n) return false;
    *v = m[at++];
    return true;
  }
  bool u16(uint32_t* v) {
    if (n - at < 2 || at > n) return false;
    *v = ((uint32_t)m[at] << 8) | m[at + 1];
    at += 2;
    return true;
  }
};

bool sampling_ok(const ilcc_jpeg_info& I) {
  if (I.n_components == 1) return true;
  const ilcc_jpeg_component* c = I.comp;
  const bool luma = (c[0].h == 1 && c[0].v == 1) || (c[0].h == 2 && c[0].v == 1) || (c[0].h == 2 && c[0].v == 2);
  return luma && c[1].h == 1 && c[1].v == 1 && c[2].h == 1 && c[2].v == 1;
}

void lay_out(ilcc_jpeg_info* I) {
  if (I->n_components == 1) {
    I->comp[0].h = I->comp[0].v = 1;   // a single-component scan is not interleaved: its factors mean nothing
    I->comp[0].blocks_w = (I->width + 7) / 8;
    I->comp[0].blocks_h = (I->height + 7) / 8;
  } else {
    const int32_t mw = (I->width + 8 * I->comp[0].h - 1) / (8 * I->comp[0].h);
    const int32_t mh = (I->height + 8 * I->comp[0].v - 1) / (8 * I->comp[0].v);
    for (int c = 0; c < 3; ++c) {
      I->comp[c].blocks_w = mw * I->comp[c].h;
      I->comp[c].blocks_h = mh * I->comp[c].v;
    }
  }
  uint64_t at = 0;
  for (int c = 0; c < I->n_components; ++c) {
    I->comp[c].coef_offset = at;
    at += (uint64_t)I->comp[c].blocks_w * (uint64_t)I->comp[c].blocks_h * 64u;
  }
  I->coef_count = at;
}

// The segments in front of the scan: fills *I, and the Huffman tables when T is given.
int32_t read_headers(const uint8_t* jpg, uint64_t bytes, ilcc_jpeg_info* I, Tables* T) {
  std::memset(I, 0, sizeof(*I));
  if (bytes < 4) return refuse("data ends early", "no SOI");
  if (jpg[0] != 0xFF || jpg[1] != 0xD8) return refuse("not a JPEG", "no SOI");
  Reader r{jpg, bytes, 2};
  bool have_sof = false, have_quant[4] = {false, false, false, false};
  uint8_t ident[3] = {0, 0, 0};
  int adobe_transform = -1;
  Tables local;
  if (!T) T = &local;
  for (;;) {
    uint32_t m = 0;
    if (r.at >= r.n) return refuse("data ends early", "no scan");
    if (jpg[r.at] != 0xFF) return refuse("not a JPEG", "marker expected");
    while (r.at < r.n && jpg[r.at] == 0xFF) ++r.at;
    if (!r.u8(&m)) return refuse("data ends early", "no scan");
    if (m == 0x00) return refuse("not a JPEG", "stuffed byte outside a scan");
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // TEM, a stray RSTn: no length
    if (m == 0xD8) return refuse("not a JPEG", "second SOI");
    if (m == 0xD9) return refuse("data ends early", "EOI before any scan");
    uint32_t length = 0;
    if (!r.u16(&length)) return refuse("data ends early", "segment length");
    if (length < 2 || length - 2 > r.n - r.at) return refuse("data ends early", "segment runs past the data");
    Reader s{jpg, r.at + length - 2, r.at};   // the segment's payload
    const uint64_t payload = length - 2;
    r.at += payload;
    switch (m) {
      case 0xC2: case 0xC5: case 0xC6: return refuse("progressive frame");
      case 0xC3: case 0xC7: return refuse("lossless frame");
      case 0xC9: case 0xCA: case 0xCB: case 0xCC: case 0xCD: case 0xCE: case 0xCF: return refuse("arithmetic coding");
      case 0xC8: return refuse("not a JPEG", "reserved frame type");
      case 0xDC: return refuse("DNL segment");
      case 0xC0:
      case 0xC1: {
        if (have_sof) return refuse("not a JPEG", "second frame header");
        uint32_t precision = 0, h = 0, w = 0, nc = 0;
        if (!s.u8(&precision) || !s.u16(&h) || !s.u16(&w) || !s.u8(&nc)) return refuse("data ends early", "SOF");
        if (precision == 12) return refuse("12-bit samples");
        if (precision != 8) return refuse("not a JPEG", "sample precision");
        if (w == 0 || h == 0) return refuse("width or height of 0");
        if (nc != 1 && nc != 3) return refuse("1 or 3 components only", nc == 2 ? "2 components" : nc == 4 ? "4 components" : "components");
        if (payload != 6 + 3 * nc) return refuse("data ends early", "SOF");
        I->width = (int32_t)w;
        I->height = (int32_t)h;
        I->n_components = (int32_t)nc;
        for (uint32_t c = 0; c < nc; ++c) {
          uint32_t id = 0, hv = 0, tq = 0;
          s.u8(&id), s.u8(&hv), s.u8(&tq);
          if (tq > 3) return refuse("not a JPEG", "quantisation table index");
          ident[c] = (uint8_t)id;
          I->comp[c].h = (int32_t)(hv >> 4);
          I->comp[c].v = (int32_t)(hv & 15);
          I->comp[c].quant_index = (int32_t)tq;
          if (I->comp[c].h < 1 || I->comp[c].h > 4 || I->comp[c].v < 1 || I->comp[c].v > 4) return refuse("unsupported sampling factors");
        }
        if (!sampling_ok(*I)) return refuse("unsupported sampling factors", "luma 1x1, 2x1 or 2x2 with chroma 1x1 only");
        have_sof = true;
        break;
      }
      case 0xDB:
        while (s.at < s.n) {
          uint32_t pt = 0;
          s.u8(&pt);
          if ((pt >> 4) == 1) return refuse("16-bit quantisation table");
          if ((pt >> 4) != 0 || (pt & 15) > 3) return refuse("not a JPEG", "DQT");
          if (s.n - s.at < 64) return refuse("data ends early", "DQT");
          for (int k = 0; k < 64; ++k) I->quant[pt & 15][kZigzag[k]] = jpg[s.at + k];
          have_quant[pt & 15] = true;
          s.at += 64;
        }
        break;
      case 0xC4:
        while (s.at < s.n) {
          uint32_t tc_th = 0;
          s.u8(&tc_th);
          const uint32_t tc = tc_th >> 4, th = tc_th & 15;
          if (tc > 1 || th > 3) return refuse("not a JPEG", "DHT");
          if (s.n - s.at < 16) return refuse("data ends early", "DHT");
          const uint8_t* counts = jpg + s.at;
          int total = 0;
          for (int k = 0; k < 16; ++k) total += counts[k];
          if (total > 256) return refuse("not a JPEG", "DHT");
          if (s.n - s.at - 16 < (uint64_t)total) return refuse("data ends early", "DHT");
          Huffman& t = tc ? T->ac[th] : T->dc[th];
          if (!t.define(counts, counts + 16, total)) return refuse("not a JPEG", "DHT over-subscribed");
          s.at += 16 + (uint64_t)total;
        }
        break;
      case 0xDD: {
        uint32_t ri = 0;
        if (payload != 2 || !s.u16(&ri)) return refuse("not a JPEG", "DRI");
        I->restart_interval = (int32_t)ri;
        break;
      }
      case 0xEE:
        if (payload >= 12 && std::memcmp(jpg + s.at, "Adobe", 5) == 0) adobe_transform = jpg[s.at + 11];
        break;
      case 0xDA: {
        if (!have_sof) return refuse("not a JPEG", "scan before the frame header");
        uint32_t ns = 0;
        if (!s.u8(&ns)) return refuse("data ends early", "SOS");
        if ((int32_t)ns != I->n_components) return refuse("several scans", "a scan that holds not all components");
        if (payload != 4 + 2 * ns) return refuse("data ends early", "SOS");
        for (uint32_t c = 0; c < ns; ++c) {
          uint32_t cs = 0, tt = 0;
          s.u8(&cs), s.u8(&tt);
          if (cs != ident[c]) return refuse("not a JPEG", "scan components out of frame order");
          ilcc_jpeg_component& k = I->comp[c];
          k.dc_table = (int32_t)(tt >> 4);
          k.ac_table = (int32_t)(tt & 15);
          if (k.dc_table > 3 || k.ac_table > 3) return refuse("not a JPEG", "Huffman table index");
          if (!have_quant[k.quant_index] || !T->dc[k.dc_table].defined || !T->ac[k.ac_table].defined)
            return refuse("table used before it is defined");
        }
        if (I->n_components == 3 && adobe_transform == 0) return refuse("Adobe transform 0", "RGB, not YCbCr");
        I->scan_offset = r.at;
        lay_out(I);
        return ILCC_OK;
      }
      default: break;   // APPn, COM and anything else with a length: skipped
    }
  }
}

// The scan's bits.  As in libjpeg any run of 0xFF bytes counts as one: followed by 0x00 it is the data byte 0xFF,
// followed by anything else it opens a marker, where the reader stops (`at` stays on the run's first byte).
struct Bits {
  const uint8_t* m;
  uint64_t n, at;
  uint64_t acc = 0;
  int nacc = 0;
  bool stopped = false;   // at a marker or at the end of the data

  void fill() {
    while (nacc <= 56 && !stopped) {
      if (at >= n) {
        stopped = true;
      } else if (m[at] != 0xFF) {
        acc = (acc << 8) | m[at++];
        nacc += 8;
      } else {
        uint64_t q = at + 1;
        while (q < n && m[q] == 0xFF) ++q;
        if (q < n && m[q] == 0x00) {
          acc = (acc << 8) | 0xFF;
          nacc += 8;
          at = q + 1;
        } else {
          stopped = true;
        }
      }
    }
  }
  uint32_t peek16() const { return (uint32_t)(nacc >= 16 ? acc >> (nacc - 16) : acc << (16 - nacc)) & 0xFFFFu; }
  uint32_t take(int k) {   // k <= nacc
    nacc -= k;
    return (uint32_t)(acc >> nacc) & ((1u << k) - 1u);
  }
  // the marker code behind the current position (entropy-coded bytes in front of it are skipped), 0: none before the end
  uint32_t next_marker() {
    nacc = 0;
    stopped = false;
    while (at < n) {
      if (m[at] != 0xFF) {
        ++at;
        continue;
      }
      uint64_t q = at + 1;
      while (q < n && m[q] == 0xFF) ++q;
      if (q >= n) break;
      at = q + 1;
      if (m[q] != 0x00) return m[q];
    }
    at = n;
    return 0;
  }
};

enum Symbol : int32_t { kEndsEarly = -1, kNoCode = -2 };

int32_t symbol(Bits& b, const Huffman& t) {
  if (b.nacc < 16) b.fill();
  const uint32_t code16 = b.peek16();
  int len = 0, sym = 0;
  if (const uint32_t e = t.look[code16 >> (16 - kLookBits)]) {
    len = (int)(e >> 8);
    sym = (int)(e & 255u);
  } else {
    for (len = kLookBits + 1; len <= 16; ++len) {
      const int32_t code = (int32_t)(code16 >> (16 - len));
      if (code <= t.maxcode[len]) {
        sym = t.values[t.first[len] + code];
        break;
      }
    }
    if (len > 16) return b.nacc < 16 ? kEndsEarly : kNoCode;
  }
  if (len > b.nacc) return kEndsEarly;
  b.nacc -= len;
  return sym;
}

// `bits` more bits as the signed value of category `bits` (T.81 F.2.2.1 EXTEND); false: the data ends first
bool receive_extend(Bits& b, int bits, int32_t* v) {
  if (b.nacc < bits) b.fill();
  if (b.nacc < bits) return false;
  const int32_t raw = (int32_t)b.take(bits);
  *v = raw >= (1 << (bits - 1)) ? raw : raw - (1 << bits) + 1;
  return true;
}

int32_t symbol_fault(int32_t s) { return s == kEndsEarly ? refuse("data ends early", "inside the scan") : refuse("Huffman code in no table"); }

}  // namespace

extern "C" {

int32_t ilcc_jpeg_parse(const uint8_t* jpg, uint64_t bytes, ilcc_jpeg_info* out) {
  if (!jpg || !out) return refuse("ilcc_jpeg_parse: null argument");
  return read_headers(jpg, bytes, out, nullptr);
}

int32_t ilcc_jpeg_layout(ilcc_jpeg_info* info) {
  if (!info) return refuse("ilcc_jpeg_layout: null argument");
  if (info->width < 1 || info->height < 1 || info->width > 65535 || info->height > 65535) return refuse("width and height must be 1 .. 65535");
  if (info->n_components != 1 && info->n_components != 3) return refuse("1 or 3 components only");
  if (!sampling_ok(*info)) return refuse("unsupported sampling factors", "luma 1x1, 2x1 or 2x2 with chroma 1x1 only");
  for (int c = 0; c < info->n_components; ++c)
    if (info->comp[c].quant_index < 0 || info->comp[c].quant_index > 3) return refuse("quantisation table index outside 0 .. 3");
  lay_out(info);
  return ILCC_OK;
}

int32_t ilcc_jpeg_entropy_decode(const uint8_t* jpg, uint64_t bytes, const ilcc_jpeg_info* info, int16_t* coef, uint64_t cap) {
  if (!jpg || !info || (!coef && cap)) return refuse("ilcc_jpeg_entropy_decode: null argument");
  ilcc_jpeg_info I;
  Tables T;
  const int32_t st = read_headers(jpg, bytes, &I, &T);
  if (st != ILCC_OK) return st;
  if (std::memcmp(&I, info, sizeof(I)) != 0) return refuse("ilcc_jpeg_entropy_decode: info is not ilcc_jpeg_parse's of these bytes");
  if (cap < I.coef_count) {
    refuse("coefficient buffer smaller than coef_count");
    return ILCC_CAPACITY;
  }
  std::memset(coef, 0, (size_t)I.coef_count * sizeof(int16_t));

  const int nc = I.n_components;
  const int32_t mcus_w = I.comp[0].blocks_w / I.comp[0].h, mcus_h = I.comp[0].blocks_h / I.comp[0].v;
  const uint64_t total = (uint64_t)mcus_w * (uint64_t)mcus_h;
  const uint64_t interval = I.restart_interval ? (uint64_t)I.restart_interval : total;
  Bits b{jpg, bytes, I.scan_offset};
  uint32_t expected_rst = 0;
  for (uint64_t mcu = 0; mcu < total;) {
    const uint64_t count = total - mcu < interval ? total - mcu : interval;
    int32_t pred[3] = {0, 0, 0};
    for (uint64_t k = mcu; k < mcu + count; ++k) {
      const int32_t my = (int32_t)(k / (uint64_t)mcus_w), mx = (int32_t)(k % (uint64_t)mcus_w);
      for (int c = 0; c < nc; ++c) {
        const ilcc_jpeg_component& C = I.comp[c];
        const Huffman& dc = T.dc[C.dc_table];
        const Huffman& ac = T.ac[C.ac_table];
        for (int dy = 0; dy < C.v; ++dy)
          for (int dx = 0; dx < C.h; ++dx) {
            int16_t* block = coef + C.coef_offset + ((uint64_t)(my * C.v + dy) * (uint64_t)C.blocks_w + (uint64_t)(mx * C.h + dx)) * 64u;
            const int32_t t = symbol(b, dc);
            if (t < 0) return symbol_fault(t);
            if (t > 15) return refuse("DC predictor leaves int16", "difference category above 15");
            int32_t diff = 0;
            if (t && !receive_extend(b, t, &diff)) return refuse("data ends early", "inside the scan");
            pred[c] += diff;
            if (pred[c] < -32768 || pred[c] > 32767) return refuse("DC predictor leaves int16");
            block[0] = (int16_t)pred[c];
            for (int at = 1; at < 64;) {
              const int32_t rs = symbol(b, ac);
              if (rs < 0) return symbol_fault(rs);
              const int run = rs >> 4, size = rs & 15;
              if (size == 0) {
                if (run != 15) break;   // EOB
                if (at + 16 > 64) return refuse("run past coefficient 63");
                at += 16;
                continue;
              }
              at += run;
              if (at > 63) return refuse("run past coefficient 63");
              int32_t v = 0;
              if (!receive_extend(b, size, &v)) return refuse("data ends early", "inside the scan");
              block[kZigzag[at++]] = (int16_t)v;   // size <= 15: |v| <= 32767
            }
          }
      }
    }
    mcu += count;
    if (mcu < total) {
      if (b.next_marker() != 0xD0u + expected_rst) return refuse("data ends early", "restart marker missing or out of order");
      expected_rst = (expected_rst + 1) & 7u;
    }
  }
  // what follows the scan: another scan or a DNL is refused, anything else (EOI, nothing) ends the image
  uint32_t m = b.next_marker();
  while (m >= 0xD0 && m <= 0xD7) m = b.next_marker();
  if (m == 0xDA) return refuse("several scans");
  if (m == 0xDC) return refuse("DNL segment");
  return ILCC_OK;
}

}  // extern "C"

int32_t ilcc::jpeg_read_headers(const uint8_t* jpg, uint64_t bytes, ilcc_jpeg_info* info, JpegTables* tables) {
  return read_headers(jpg, bytes, info, tables);
}

bool ilcc::jpeg_laid_out(const ilcc_jpeg_info& I) {
  ilcc_jpeg_info L = I;
  if (ilcc_jpeg_layout(&L) != ILCC_OK) return false;
  return std::memcmp(&L, &I, sizeof(L)) == 0;
}
