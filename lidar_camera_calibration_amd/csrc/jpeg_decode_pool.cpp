// ilcc_jpeg_entropy_decode_many (include/ilcc_jpeg_sequence.h): the Huffman decode of a batch of JPEG files on several host
// threads.  Plain C++ without HIP; it builds alone with csrc/jpeg_entropy.cpp (under ThreadSanitizer and AddressSanitizer
// for tests/test_jpeg_sequence_cpu.py).  ilcc_jpeg_entropy_decode allocates nothing, writes only its own coef[] and keeps its
// error text per thread, so the jobs share nothing but the counter they are drawn from: a job's result is the same on
// whichever thread it runs.  The calling thread is one of the workers.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "ilcc_hip.h"
#include "ilcc_jpeg_sequence.h"
#include "jpeg_entropy.h"

namespace {

constexpr uint32_t kDefaultThreads = 8, kMaxThreads = 16;   // never hardware_concurrency: a shared machine shows all its cores

struct Pool {
  const uint8_t* const* jpg;
  const uint64_t* bytes;
  const ilcc_jpeg_info* info;
  int16_t* const* coef;
  const uint64_t* cap;
  int32_t* status;
  uint32_t n;
  std::atomic<uint32_t> next{0};
  std::mutex mutex;            // guards the two below
  uint32_t lowest_failed;      // n: none
  char text[160];

  void work() {
    for (uint32_t i; (i = next.fetch_add(1, std::memory_order_relaxed)) < n;) {
      const int32_t st = ilcc_jpeg_entropy_decode(jpg[i], bytes[i], &info[i], coef[i], cap[i]);
      status[i] = st;
      if (st == ILCC_OK) continue;
      std::lock_guard<std::mutex> lock(mutex);
      if (i < lowest_failed) {
        lowest_failed = i;
        std::snprintf(text, sizeof(text), "%s", ilcc::jpeg_last_error());   // this thread's text, of this job
      }
    }
  }
};

// joins whatever makes the call end
struct Threads {
  std::vector<std::thread> t;
  ~Threads() {
    for (std::thread& x : t)
      if (x.joinable()) x.join();
  }
};

}  // namespace

extern "C" int32_t ilcc_jpeg_entropy_decode_many(const uint8_t* const* jpg, const uint64_t* bytes, const ilcc_jpeg_info* info,
                                                 int16_t* const* coef, const uint64_t* cap, uint32_t n, uint32_t threads, int32_t* status) {
  if (n == 0) return ILCC_OK;
  if (!jpg || !bytes || !info || !coef || !cap || !status) return ilcc::jpeg_refuse("ilcc_jpeg_entropy_decode_many: null argument");
  Pool pool;
  pool.jpg = jpg;
  pool.bytes = bytes;
  pool.info = info;
  pool.coef = coef;
  pool.cap = cap;
  pool.status = status;
  pool.n = n;
  pool.lowest_failed = n;
  pool.text[0] = 0;
  uint32_t count = threads ? threads : kDefaultThreads;
  if (count > kMaxThreads) count = kMaxThreads;
  if (count > n) count = n;
  {
    Threads others;
    try {
      others.t.reserve(count - 1);
      for (uint32_t k = 1; k < count; ++k) others.t.emplace_back([&pool] { pool.work(); });
    } catch (...) {
      // fewer threads than asked for: the ones that started and this one take all the jobs
    }
    pool.work();
  }   // joined
  if (pool.lowest_failed == n) return ILCC_OK;
  // the lowest failing job's text becomes the calling thread's
  if (ilcc::jpeg_error_sink) ilcc::jpeg_error_sink(pool.text);
  return status[pool.lowest_failed];
}
