// paired_host.cpp -- the host-only layers of include/ilcc_paired.h: ilcc_pair_by_stamp (the image of every cloud, by header
// stamp) and ilcc_save_pcd_xyzrgb (the binary PCD file of an XYZRGB cloud).  Plain C++ without HIP; it also builds alone, under
// sanitizers, for tests/test_paired_cpu.py.  tests/paired_ref.py restates both.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <new>
#include <numeric>
#include <vector>

#include "ilcc_paired.h"

namespace {

struct Nearest {
  uint64_t abs_dt;
  bool image_later;   // image_ns >= cloud_ns
  uint64_t j;
};

inline Nearest distance_to(uint64_t cloud, uint64_t image, uint64_t j) {
  return image >= cloud ? Nearest{image - cloud, true, j} : Nearest{cloud - image, false, j};   // unsigned: no wrap at any stamp
}

}  // namespace

extern "C" {

int32_t ilcc_pair_by_stamp(const uint64_t* cloud_ns, uint64_t n_clouds, const uint64_t* image_ns, uint64_t n_images, uint64_t max_dt_ns,
                           int64_t* image_of, int64_t* dt_ns) {
  if ((n_clouds && (!cloud_ns || !image_of || !dt_ns)) || (n_images && !image_ns)) return ILCC_BAD_ARGUMENT;
  if (n_images == 0) {
    for (uint64_t i = 0; i < n_clouds; ++i) {
      image_of[i] = -1;
      dt_ns[i] = 0;
    }
    return ILCC_OK;
  }
  // the image indices by stamp; stable, so that equal stamps stand in index order and the first of a run is the lowest j
  std::vector<uint64_t> order;
  try {
    order.resize(n_images);
  } catch (const std::bad_alloc&) {   // no exception crosses the C-ABI
    return ILCC_IO_ERROR;
  }
  std::iota(order.begin(), order.end(), (uint64_t)0);
  std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return image_ns[a] < image_ns[b]; });
  const auto first_not_below = [&](uint64_t stamp) {
    return std::lower_bound(order.begin(), order.end(), stamp, [&](uint64_t j, uint64_t v) { return image_ns[j] < v; });
  };
  for (uint64_t i = 0; i < n_clouds; ++i) {
    const uint64_t c = cloud_ns[i];
    const auto at = first_not_below(c);
    Nearest best{};
    bool have = false;
    if (at != order.end()) {   // the earliest image not before the cloud, lowest index among equal stamps
      best = distance_to(c, image_ns[*at], *at);
      have = true;
    }
    if (at != order.begin()) {   // the latest image before the cloud: the first of its run of equal stamps
      const uint64_t stamp = image_ns[*(at - 1)];
      const uint64_t j = *first_not_below(stamp);
      const Nearest left = distance_to(c, stamp, j);
      if (!have || left.abs_dt < best.abs_dt || (left.abs_dt == best.abs_dt && left.j < best.j)) best = left;
    }
    const bool fits = best.abs_dt <= (uint64_t)INT64_MAX;
    dt_ns[i] = best.image_later ? (fits ? (int64_t)best.abs_dt : INT64_MAX) : (fits ? -(int64_t)best.abs_dt : INT64_MIN);
    image_of[i] = (fits && best.abs_dt <= max_dt_ns) ? (int64_t)best.j : -1;
  }
  return ILCC_OK;
}

int32_t ilcc_save_pcd_xyzrgb(const char* filename, const void* xyzrgb, uint64_t n) {
  if (!filename || (n && !xyzrgb)) return ILCC_BAD_ARGUMENT;
  FILE* f = std::fopen(filename, "wb");
  if (!f) return ILCC_IO_ERROR;
  bool ok = std::fprintf(f,
                         "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\n"
                         "COUNT 1 1 1 1\nWIDTH %" PRIu64 "\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %" PRIu64 "\nDATA binary\n",
                         n, n) > 0;
  if (ok && n) ok = std::fwrite(xyzrgb, 16, n, f) == n;
  ok = (std::fclose(f) == 0) && ok;
  return ok ? ILCC_OK : ILCC_IO_ERROR;
}

}  // extern "C"
