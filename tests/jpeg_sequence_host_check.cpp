// Stand-alone check of csrc/jpeg_decode_pool.cpp, built by tests/test_jpeg_sequence_cpu.py with -fsanitize=thread and again
// with -fsanitize=address,undefined, and linked with that file and csrc/jpeg_entropy.cpp only:
//
//   jpeg_sequence_host_check dump.bin intact.jpg ... -- corrupt.jpg ...
//
// The files behind "--" parse but their scans do not decode.  They are interleaved with the intact ones (one corrupt job after
// every fifth intact one, the rest at the end) and all jobs go through ilcc_jpeg_entropy_decode_many on 1, 4 and 16 threads.
// Every time: an intact job's status is ILCC_OK, a corrupt one's ILCC_BAD_ARGUMENT; the return value is the lowest failing
// job's status and the text handed to the error sink on the calling thread is what ilcc_jpeg_entropy_decode says of that job
// alone; the intact jobs' coefficients are byte for byte those of the run on one thread.  Those go to dump.bin, per intact
// file a uint64 count and that many int16.  Each input and each output sits in a heap block of exactly its size.  Exit
// status 0: all held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ilcc_hip.h"
#include "ilcc_jpeg_sequence.h"
#include "jpeg_entropy.h"

namespace {

thread_local char t_text[160] = "";   // the sink is called on whichever thread refuses

void sink(const char* text) { std::snprintf(t_text, sizeof(t_text), "%s", text); }

struct Job {
  std::string path;
  bool intact = true;
  uint8_t* jpg = nullptr;   // exactly `bytes`
  uint64_t bytes = 0;
  ilcc_jpeg_info info{};
  int16_t* coef = nullptr;  // exactly coef_count
};

bool load(Job* j) {
  FILE* f = std::fopen(j->path.c_str(), "rb");
  if (!f) return false;
  std::vector<uint8_t> all;
  uint8_t buf[4096];
  for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) all.insert(all.end(), buf, buf + n);
  std::fclose(f);
  if (all.empty()) return false;
  j->bytes = all.size();
  j->jpg = (uint8_t*)std::malloc(all.size());
  std::memcpy(j->jpg, all.data(), all.size());
  if (ilcc_jpeg_parse(j->jpg, j->bytes, &j->info) != ILCC_OK) return false;
  j->coef = (int16_t*)std::malloc(j->info.coef_count * sizeof(int16_t));
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  ilcc::jpeg_error_sink = sink;
  std::vector<Job> intact, corrupt;
  int at = 2;
  for (; at < argc && std::strcmp(argv[at], "--") != 0; ++at) {
    Job j;
    j.path = argv[at];
    intact.push_back(j);
  }
  for (++at; at < argc; ++at) {
    Job j;
    j.path = argv[at];
    j.intact = false;
    corrupt.push_back(j);
  }
  std::vector<Job> jobs;
  size_t next_corrupt = 0;
  for (size_t i = 0; i < intact.size(); ++i) {
    jobs.push_back(intact[i]);
    if (i % 5 == 4 && next_corrupt < corrupt.size()) jobs.push_back(corrupt[next_corrupt++]);
  }
  for (; next_corrupt < corrupt.size(); ++next_corrupt) jobs.push_back(corrupt[next_corrupt]);
  for (Job& j : jobs)
    if (!load(&j)) {
      std::fprintf(stderr, "%s: can not be read or its headers do not parse\n", j.path.c_str());
      return 2;
    }
  const uint32_t n = (uint32_t)jobs.size();
  std::vector<const uint8_t*> jpg(n);
  std::vector<uint64_t> bytes(n), cap(n);
  std::vector<ilcc_jpeg_info> info(n);
  std::vector<int16_t*> coef(n);
  for (uint32_t i = 0; i < n; ++i) {
    jpg[i] = jobs[i].jpg;
    bytes[i] = jobs[i].bytes;
    info[i] = jobs[i].info;
    coef[i] = jobs[i].coef;
    cap[i] = jobs[i].info.coef_count;
  }
  uint32_t lowest = n;
  for (uint32_t i = n; i-- > 0;)
    if (!jobs[i].intact) lowest = i;
  std::vector<std::vector<int16_t>> first_run(n);
  const uint32_t thread_counts[3] = {1, 4, 16};
  for (int round = 0; round < 3; ++round) {
    for (uint32_t i = 0; i < n; ++i) std::memset(coef[i], 0x5A, cap[i] * sizeof(int16_t));
    std::vector<int32_t> status(n, -77);
    t_text[0] = 0;
    const int32_t st = ilcc_jpeg_entropy_decode_many(jpg.data(), bytes.data(), info.data(), coef.data(), cap.data(), n, thread_counts[round], status.data());
    const std::string got_text = t_text;
    for (uint32_t i = 0; i < n; ++i)
      if (status[i] != (jobs[i].intact ? ILCC_OK : ILCC_BAD_ARGUMENT)) {
        std::fprintf(stderr, "%s on %u threads: status %d\n", jobs[i].path.c_str(), thread_counts[round], status[i]);
        return 1;
      }
    if (st != (lowest < n ? ILCC_BAD_ARGUMENT : ILCC_OK)) {
      std::fprintf(stderr, "%u threads: returned %d\n", thread_counts[round], st);
      return 1;
    }
    if (lowest < n) {   // the text is the lowest failing job's own
      std::vector<int16_t> scratch(cap[lowest]);
      (void)ilcc_jpeg_entropy_decode(jpg[lowest], bytes[lowest], &info[lowest], scratch.data(), scratch.size());
      if (got_text.empty() || got_text != ilcc::jpeg_last_error()) {
        std::fprintf(stderr, "%u threads: text '%s', the lowest failing job's is '%s'\n", thread_counts[round], got_text.c_str(), ilcc::jpeg_last_error());
        return 1;
      }
    }
    for (uint32_t i = 0; i < n; ++i) {
      if (!jobs[i].intact) continue;
      if (round == 0) first_run[i].assign(coef[i], coef[i] + cap[i]);
      else if (std::memcmp(first_run[i].data(), coef[i], cap[i] * sizeof(int16_t)) != 0) {
        std::fprintf(stderr, "%s: coefficients on %u threads differ from those on one\n", jobs[i].path.c_str(), thread_counts[round]);
        return 1;
      }
    }
  }
  // n == 0 and null arrays
  if (ilcc_jpeg_entropy_decode_many(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 4, nullptr) != ILCC_OK) return 1;
  if (ilcc_jpeg_entropy_decode_many(nullptr, bytes.data(), info.data(), coef.data(), cap.data(), n, 4, nullptr) != ILCC_BAD_ARGUMENT) return 1;
  FILE* dump = std::fopen(argv[1], "wb");
  if (!dump) return 2;
  for (uint32_t i = 0; i < n; ++i) {
    if (!jobs[i].intact) continue;
    const uint64_t count = first_run[i].size();
    std::fwrite(&count, sizeof(count), 1, dump);
    std::fwrite(first_run[i].data(), sizeof(int16_t), first_run[i].size(), dump);
  }
  std::fclose(dump);
  for (Job& j : jobs) {
    std::free(j.jpg);
    std::free(j.coef);
  }
  std::printf("%u jobs (%zu corrupt) on 1, 4 and 16 threads: statuses, text and coefficients as on one thread\n", n, corrupt.size());
  return 0;
}
