// Stand-alone check of csrc/jpeg_entropy.cpp, built by tests/test_jpeg_cpu.py with -fsanitize=address,undefined and
// linked with that file only:
//
//   jpeg_host_check dump.bin intact.jpg ... -- small.jpg ...
//
// Every file in front of "--" must parse and decode (ILCC_OK); its coefficients go to dump.bin as a uint64 count and
// that many int16.  Every file behind it is decoded again as each of its prefixes and with each single byte set to 0x00
// and to 0xFF; every call must return ILCC_OK or ILCC_BAD_ARGUMENT.  Each input sits in a heap block of exactly its
// size, so a read past `bytes` is a sanitizer report.  Exit status 0: all held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ilcc_hip.h"
#include "ilcc_jpeg.h"

namespace {

std::vector<uint8_t> file_bytes(const char* path) {
  std::vector<uint8_t> out;
  FILE* f = std::fopen(path, "rb");
  if (!f) return out;
  uint8_t buf[4096];
  for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) out.insert(out.end(), buf, buf + n);
  std::fclose(f);
  return out;
}

// parse + decode of exactly `n` bytes; the status of the step that ended it
int32_t decode(const uint8_t* data, size_t n, std::vector<int16_t>* coef) {
  uint8_t* exact = (uint8_t*)std::malloc(n ? n : 1);
  if (n) std::memcpy(exact, data, n);
  ilcc_jpeg_info info;
  int32_t st = ilcc_jpeg_parse(exact, n, &info);
  if (st == ILCC_OK) {
    if (info.coef_count > (64u << 20)) {   // a mutated size field: the headers are checked, the scan is not worth the memory
      std::free(exact);
      return ILCC_OK;
    }
    int16_t* out = (int16_t*)std::malloc(info.coef_count * sizeof(int16_t) + 2);   // exactly coef_count: a write past it is a report
    st = ilcc_jpeg_entropy_decode(exact, n, &info, out, info.coef_count);
    if (coef) coef->assign(out, out + info.coef_count);
    std::free(out);
  }
  std::free(exact);
  return st;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* dump = std::fopen(argv[1], "wb");
  if (!dump) return 2;
  int at = 2;
  for (; at < argc && std::strcmp(argv[at], "--") != 0; ++at) {
    const std::vector<uint8_t> jpg = file_bytes(argv[at]);
    std::vector<int16_t> coef;
    const int32_t st = decode(jpg.data(), jpg.size(), &coef);
    if (st != ILCC_OK) {
      std::fprintf(stderr, "%s: status %d\n", argv[at], st);
      return 1;
    }
    const uint64_t count = coef.size();
    std::fwrite(&count, sizeof(count), 1, dump);
    std::fwrite(coef.data(), sizeof(int16_t), coef.size(), dump);
  }
  std::fclose(dump);
  long calls = 0;
  for (++at; at < argc; ++at) {
    std::vector<uint8_t> jpg = file_bytes(argv[at]);
    if (jpg.empty()) return 2;
    auto check = [&](size_t n, const char* what, size_t where) {
      const int32_t st = decode(jpg.data(), n, nullptr);
      ++calls;
      if (st == ILCC_OK || st == ILCC_BAD_ARGUMENT) return true;
      std::fprintf(stderr, "%s: %s %zu: status %d\n", argv[at], what, where, st);
      return false;
    };
    for (size_t n = 0; n < jpg.size(); ++n)
      if (!check(n, "prefix", n)) return 1;
    for (size_t i = 0; i < jpg.size(); ++i)
      for (int v = 0; v < 2; ++v) {
        const uint8_t keep = jpg[i];
        jpg[i] = v ? 0xFF : 0x00;
        const bool ok = check(jpg.size(), v ? "byte set to 0xFF at" : "byte set to 0x00 at", i);
        jpg[i] = keep;
        if (!ok) return 1;
      }
  }
  std::printf("%ld mutated inputs: every status ILCC_OK or ILCC_BAD_ARGUMENT\n", calls);
  return 0;
}
