// Stand-alone check of csrc/jpeg_entropy_enc.cpp, built by tests/test_jpeg_write_cpu.py with -fsanitize=address,undefined
// and linked with that file and csrc/jpeg_entropy.cpp only:
//
//   jpeg_write_host_check cases.bin
//
// cases.bin holds, per case, seven int32 (width, height, components, sampling h, v, quality, restart interval), a uint64
// count and that many int16 coefficients, a uint64 size and that many bytes: the file libjpeg writes for them.  For
// every case the encoder must reproduce the file in a heap block of exactly its size, the decoder must give the
// coefficients back, every shorter `cap` (each one for files below 700 bytes, a spread of them above) must answer
// ILCC_CAPACITY into a heap block of exactly `cap` bytes, so that a write past it is a sanitizer report, and
// ilcc_jpeg_file_bound must hold.  On the first case, coefficients at and past libjpeg's limits: DC differences of
// +-2047 and AC values of +-1023 must encode and decode back, +-2048 and +-1024 must answer ILCC_BAD_ARGUMENT.
// Exit status 0: all held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ilcc_hip.h"
#include "ilcc_jpeg_write.h"
#include "jpeg_entropy.h"

namespace {

struct Case {
  int32_t head[7];
  std::vector<int16_t> coef;
  std::vector<uint8_t> file;
};

bool read_case(FILE* f, Case* c) {
  uint64_t n = 0;
  if (std::fread(c->head, sizeof(int32_t), 7, f) != 7) return false;
  if (std::fread(&n, sizeof(n), 1, f) != 1) return false;
  c->coef.resize(n);
  if (n && std::fread(c->coef.data(), sizeof(int16_t), n, f) != n) return false;
  if (std::fread(&n, sizeof(n), 1, f) != 1) return false;
  c->file.resize(n);
  return std::fread(c->file.data(), 1, n, f) == n;
}

// encode into a heap block of exactly `cap` bytes
int32_t encode(const ilcc_jpeg_info& info, const std::vector<int16_t>& coef, uint64_t cap, std::vector<uint8_t>* got, uint64_t* bytes) {
  int16_t* in = (int16_t*)std::malloc(coef.size() * sizeof(int16_t) + 1);   // exactly coef_count: a read past it is a report
  std::memcpy(in, coef.data(), coef.size() * sizeof(int16_t));
  uint8_t* out = (uint8_t*)std::malloc(cap ? cap : 1);
  const int32_t st = ilcc_jpeg_entropy_encode(&info, in, out, cap, bytes);
  if (got && st == ILCC_OK) got->assign(out, out + *bytes);
  std::free(out);
  std::free(in);
  return st;
}

bool decodes_back(const std::vector<uint8_t>& file, const std::vector<int16_t>& coef) {
  ilcc_jpeg_info parsed;
  if (ilcc_jpeg_parse(file.data(), file.size(), &parsed) != ILCC_OK || parsed.coef_count != coef.size()) return false;
  std::vector<int16_t> back(coef.size() + 1);
  if (ilcc_jpeg_entropy_decode(file.data(), file.size(), &parsed, back.data(), coef.size()) != ILCC_OK) return false;
  return std::memcmp(back.data(), coef.data(), coef.size() * sizeof(int16_t)) == 0;
}

int fail(int index, const char* what, long detail = 0) {
  std::fprintf(stderr, "case %d: %s (%ld): %s\n", index, what, detail, ilcc::jpeg_last_error());
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int index = 0;
  long short_caps = 0;
  Case c, first;
  for (; read_case(f, &c); ++index) {
    ilcc_jpeg_info info;
    const int32_t* h = c.head;
    if (ilcc_jpeg_write_info(h[0], h[1], h[2], h[3], h[4], h[5], h[6], &info) != ILCC_OK) return fail(index, "write_info");
    if (info.coef_count != c.coef.size()) return fail(index, "coef_count", (long)info.coef_count);
    if (ilcc_jpeg_file_bound(&info) < c.file.size()) return fail(index, "file_bound", (long)ilcc_jpeg_file_bound(&info));
    std::vector<uint8_t> got;
    uint64_t bytes = 0;
    if (encode(info, c.coef, c.file.size(), &got, &bytes) != ILCC_OK) return fail(index, "encode into the exact size");
    if (got != c.file) return fail(index, "file bytes differ", (long)bytes);
    if (!decodes_back(got, c.coef)) return fail(index, "decode(encode(c)) != c");
    const uint64_t step = c.file.size() < 700 ? 1 : c.file.size() / 61;
    for (uint64_t cap = 0; cap < c.file.size(); cap += step, ++short_caps) {
      bytes = 77;
      if (encode(info, c.coef, cap, nullptr, &bytes) != ILCC_CAPACITY || bytes != 0) return fail(index, "short cap", (long)cap);
    }
    if (encode(info, c.coef, c.file.size() - 1, nullptr, &bytes) != ILCC_CAPACITY) return fail(index, "cap one short");
    if (index == 0) first = c;
  }
  std::fclose(f);
  if (index == 0) return 2;

  // libjpeg's limits, on the first case's info with all coefficients zero but one
  ilcc_jpeg_info info;
  const int32_t* h = first.head;
  if (ilcc_jpeg_write_info(h[0], h[1], h[2], h[3], h[4], h[5], 0, &info) != ILCC_OK) return fail(-1, "write_info");
  const uint64_t bound = ilcc_jpeg_file_bound(&info);
  const struct {
    int k;
    int value;
    int32_t want;
  } limits[] = {{0, 2047, ILCC_OK},  {0, -2047, ILCC_OK},  {0, 2048, ILCC_BAD_ARGUMENT},  {0, -2048, ILCC_BAD_ARGUMENT},
                {0, 32767, ILCC_BAD_ARGUMENT}, {0, -32768, ILCC_BAD_ARGUMENT},
                {1, 1023, ILCC_OK},  {1, -1023, ILCC_OK},  {1, 1024, ILCC_BAD_ARGUMENT},  {1, -1024, ILCC_BAD_ARGUMENT},
                {63, 1023, ILCC_OK}, {63, -1023, ILCC_OK}, {63, 1024, ILCC_BAD_ARGUMENT}, {63, -32768, ILCC_BAD_ARGUMENT}};
  for (const auto& l : limits) {
    std::vector<int16_t> coef(info.coef_count, 0);
    coef[(size_t)l.k] = (int16_t)l.value;
    std::vector<uint8_t> got;
    uint64_t bytes = 0;
    const int32_t st = encode(info, coef, bound, &got, &bytes);
    if (st != l.want) return fail(-1, "limit", l.value);
    if (st == ILCC_OK && !decodes_back(got, coef)) return fail(-1, "limit does not decode back", l.value);
    if (st != ILCC_OK && bytes != 0) return fail(-1, "bytes set by a refusal", l.value);
  }
  // a worst-case block: every coefficient at the limit, alternating sign, must fit the bound
  {
    std::vector<int16_t> coef(info.coef_count);
    for (size_t k = 0; k < coef.size(); ++k) coef[k] = (int16_t)((k & 1) ? -1023 : 1023);
    for (size_t b = 0; b < coef.size(); b += 64) coef[b] = (int16_t)((b & 64) ? -1023 : 1023);
    std::vector<uint8_t> got;
    uint64_t bytes = 0;
    if (encode(info, coef, bound, &got, &bytes) != ILCC_OK || !decodes_back(got, coef)) return fail(-1, "worst case within file_bound");
  }
  std::printf("%d cases, %ld short caps: every file reproduced, decoded back and bounded\n", index, short_caps);
  return 0;
}
