// paired_api.cpp -- ilcc_bag_rgblidar_all_scans (include/ilcc_paired.h): every selected scan of a recording coloured from the image
// whose header stamp is nearest to its own.  The recording, its batches (cut BEFORE anything is allocated, so the buffers are sized
// by the largest batch, not by the budgets), the staging and the upload with K0b and K11c are the paired front end's
// (paired_front.h); an unpaired scan is staged and unpacked like any other.  This file owns K8b (k8b_colourise_batch.hip) with its
// records, and the order of the calls that lets the host stage the next batch while the device works on this one.  Failures below
// are reported through ilcc_last_error(NULL).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "paired_front.h"

using namespace ilcc;

namespace {

constexpr uint64_t kDefaultMaxDtNs = 50000000ull;

// one of the two sets of buffers
struct Buffers : PairedBuffers {
  Pinned h_records;
  DeviceBuffer d_records;
  ilcc_colourise_plan* colour = nullptr;
  std::vector<uint64_t> out_offsets;
  ~Buffers() { ilcc_colourise_plan_destroy(colour); }
};

int32_t all_scans(int32_t device, const char* image_bag, const char* image_topic, const char* lidar_bag, const char* lidar_topic,
                  const ilcc_camera_model* camera, const double* T, double distance_valid, const ilcc_paired_params& pp, ilcc_pair_sink sink,
                  void* user, uint32_t* n_scans, uint32_t* n_paired) {
  PairedRecording c;
  int32_t st = c.open("ilcc_bag_rgblidar_all_scans", image_bag, image_topic, lidar_bag, lidar_topic, camera, T, pp.first, pp.stride, pp.max_scans, pp.max_dt_ns);
  if (st != ILCC_OK) return st;
  *n_scans = (uint32_t)c.selected.size();
  *n_paired = c.n_paired();
  std::vector<PairedBatch> batches;
  PairedLargest largest;
  PairedBudgets budgets;
  budgets.staging = pp.staging_bytes;
  budgets.image = pp.image_bytes;
  budgets.stage_unpaired = true;
  if ((st = c.cut(budgets, &batches, &largest)) != ILCC_OK) return st;

  // one set of allocations for the whole call
  if ((st = select_device(device)) != ILCC_OK) return st;
  hipError_t e;
  Stream stream;
  if ((e = hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking)) != hipSuccess) return hip_fail(e);
  Buffers B[2];
  const int sets = batches.size() > 1 ? 2 : 1;
  const uint64_t points = std::max<uint64_t>(largest.points, 1);
  for (int k = 0; k < sets; ++k) {
    Buffers& b = B[k];
    if ((st = b.allocate(largest)) != ILCC_OK) return st;
    if ((e = hipHostMalloc((void**)&b.h_records.p, 16 * points, hipHostMallocDefault)) != hipSuccess || (e = hipMalloc(&b.d_records.p, 16 * points)) != hipSuccess)
      return hip_fail(e);
    if (!(b.colour = ilcc_colourise_plan_create(largest.members, points))) return ILCC_HIP_ERROR;
  }
  InFlight flying;   // declared behind the buffers: its destructor runs before theirs
  flying.s = stream.s;

  // everything the device does for the batch B carries, queued on the stream
  const auto submit = [&](Buffers* B) -> int32_t {
    PairedImages im;
    const int32_t s = c.upload(B, pp.sample_raw ? nullptr : camera, stream.s, &im);
    if (s != ILCC_OK) return s;
    return ilcc_colourise_batch_device(B->d_xyzi.p, B->offsets.data(), B->batch->scans, im.image_ptrs.data(), im.steps.data(), (uint32_t)im.image_ptrs.size(),
                                       im.image_of_scan.data(), &c.proj, distance_valid, B->d_records.p, B->batch->points, B->colour, stream.s);
  };

  // the batches: while the device works on batch k the host reads, inflates and stages batch k + 1
  if ((st = c.stage(&B[0], batches[0])) != ILCC_OK || (st = submit(&B[0])) != ILCC_OK) return st;
  for (size_t k = 0; k < batches.size(); ++k) {
    Buffers& now = B[k & 1];
    Buffers& next = B[(k + 1) & 1];   // its previous batch has been finished, copied back and handed to the sink
    const bool more = k + 1 < batches.size();
    int32_t st_next = more ? c.stage(&next, batches[k + 1]) : ILCC_OK;
    const PairedBatch& b = *now.batch;
    now.out_offsets.assign(b.scans + 1, 0);
    if ((st = ilcc_colourise_plan_finish(now.colour, now.out_offsets.data())) != ILCC_OK) return st;
    if (st_next != ILCC_OK) return st_next;
    if (more && (st = submit(&next)) != ILCC_OK) return st;   // the device goes on while the host copies back and sinks
    const uint64_t total = now.out_offsets[b.scans];
    if (total && (e = hipMemcpy(now.h_records.p, now.d_records.p, 16 * total, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e);
    for (uint32_t s = 0; s < b.scans; ++s) {
      const uint32_t g = b.first_scan + s;
      ilcc_pair_record r;
      c.fill(g, &r);
      r.n_coloured = now.out_offsets[s + 1] - now.out_offsets[s];
      if (sink && sink(user, &r, now.h_records.p + 16 * now.out_offsets[s]) != 0) return fail(ILCC_IO_ERROR, "the sink refused scan " + std::to_string(g));
    }
  }
  return ILCC_OK;
}

}  // namespace

extern "C" {

void ilcc_default_paired_params(ilcc_paired_params* pp) {
  if (!pp) return;
  std::memset(pp, 0, sizeof(*pp));
  pp->stride = 1;
  pp->max_dt_ns = kDefaultMaxDtNs;
  pp->staging_bytes = kDefaultPairedStagingBytes;
  pp->image_bytes = kDefaultPairedImageBytes;
}

int32_t ilcc_bag_rgblidar_all_scans(int32_t device, const char* image_bag, const char* image_topic, const char* lidar_bag, const char* lidar_topic,
                                    const ilcc_camera_model* camera, const double T_lidar2cam[16], double distance_valid, const ilcc_paired_params* pp,
                                    ilcc_pair_sink sink, void* user, uint32_t* n_scans, uint32_t* n_paired) {
  if (!image_bag || !image_topic || !lidar_bag || !lidar_topic || !camera || !T_lidar2cam || !n_scans || !n_paired)
    return fail(ILCC_BAD_ARGUMENT, "ilcc_bag_rgblidar_all_scans: null argument");
  *n_scans = *n_paired = 0;
  ilcc_paired_params defaults;
  ilcc_default_paired_params(&defaults);
  try {   // no exception crosses the C-ABI
    return all_scans(device, image_bag, image_topic, lidar_bag, lidar_topic, camera, T_lidar2cam, distance_valid, pp ? *pp : defaults, sink, user, n_scans,
                     n_paired);
  } catch (const std::bad_alloc&) {
    return fail(ILCC_IO_ERROR, "out of memory");
  } catch (...) {
    return fail(ILCC_IO_ERROR, "paired: unknown failure");
  }
}

}  // extern "C"
