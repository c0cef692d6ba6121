// paired_api.cpp -- ilcc_bag_rgblidar_all_scans (include/ilcc_paired.h): every selected scan of a recording coloured from the image
// whose header stamp is nearest to its own.  The layers below do the work: the topic iterator (bag_reader.cpp), the pairing
// (paired_host.cpp), K0b (k0b_unpack_batch.hip), K11c (k11_camera_image.hip), K8b (k8b_colourise_batch.hip).  This file owns the
// batching: it reads every header once, cuts the selected scans into batches by the two budgets BEFORE anything is allocated (so
// the buffers are sized by the largest batch, not by the budgets), and runs the batches through two sets of buffers so that the
// host stages the next batch while the device works on this one.  Failures below are reported through ilcc_last_error(NULL).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "host_util.h"
#include "ilcc_paired.h"

using namespace ilcc;

namespace {

constexpr uint64_t kDefaultStagingBytes = 256ull << 20, kDefaultImageBytes = 512ull << 20, kDefaultMaxDtNs = 50000000ull;
constexpr const char* kImageMd5 = "060021388200f6f0f447d0fcd9c64743";
constexpr const char* kCompressedImageMd5 = "8f7a12909da2c9d3332d540a0977563f";

inline uint64_t align16(uint64_t v) { return (v + 15u) & ~(uint64_t)15u; }
inline uint64_t stamp_ns(uint32_t sec, uint32_t nsec) { return (uint64_t)sec * 1000000000ull + nsec; }

struct Iterator {
  ilcc_bag_topic* it = nullptr;
  ~Iterator() { ilcc_bag_topic_close(it); }
};
struct Stream {
  hipStream_t s = nullptr;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
};
struct Pinned {
  uint8_t* p = nullptr;
  ~Pinned() {
    if (p) (void)hipHostFree(p);
  }
};
// whatever made the call end, the stream's work must have finished before the buffers it uses go away
struct InFlight {
  hipStream_t s = nullptr;
  ~InFlight() {
    if (s) (void)hipStreamSynchronize(s);
  }
};

// the message `i` of the topic in `msg`
int32_t read_message(ilcc_bag_topic* it, uint64_t i, std::vector<uint8_t>* msg, uint64_t* bytes) {
  int32_t st = ilcc_bag_topic_read(it, i, nullptr, 0, bytes);
  if (st != ILCC_OK && st != ILCC_CAPACITY) return st;
  msg->resize(*bytes ? *bytes : 1);
  return ilcc_bag_topic_read(it, i, msg->data(), *bytes, bytes);
}

struct ImageSlot {      // a distinct image of a batch
  uint32_t image;       // index on the topic
  uint64_t raw_at, bgr_at;   // in the batch's raw / B,G,R regions
};

struct Batch {
  uint32_t first_scan = 0, scans = 0;   // among the selected scans
  uint64_t blob_bytes = 0, points = 0, raw_bytes = 0, bgr_bytes = 0;
  std::vector<ImageSlot> images;
};

// one of the two sets of buffers
struct Buffers {
  Pinned h_blob, h_raw, h_records;
  DeviceBuffer d_blob, d_xyzi, d_raw, d_bgr, d_records;
  ilcc_unpack_plan* unpack = nullptr;
  ilcc_colourise_plan* colour = nullptr;
  std::vector<uint64_t> src, offsets, out_offsets;
  const Batch* batch = nullptr;
  ~Buffers() {
    ilcc_unpack_plan_destroy(unpack);
    ilcc_colourise_plan_destroy(colour);
  }
};

struct Chain {
  ilcc_bag_topic* clouds = nullptr;
  ilcc_bag_topic* images = nullptr;
  std::vector<uint64_t> selected;                  // cloud message indices
  std::vector<ilcc_pointcloud2_layout> cloud_of;   // per selected scan
  std::vector<ilcc_image_layout> image_of_topic;   // per image message
  std::vector<int64_t> pair, dt;                   // per selected scan
  std::vector<Batch> batches;
  std::vector<uint8_t> msg;
  const ilcc_camera_model* camera = nullptr;
  bool sample_raw = false;
  ilcc_projection proj{};
  double distance_valid = 0;
  uint64_t bgr_image_bytes = 0;

  // host only: the batch's messages into the page-locked buffers
  int32_t stage(Buffers* B, const Batch& b) {
    B->batch = &b;
    B->src.clear();
    uint64_t at = 0, bytes = 0;
    for (uint32_t k = 0; k < b.scans; ++k) {
      const ilcc_pointcloud2_layout& L = cloud_of[b.first_scan + k];
      const int32_t st = read_message(clouds, selected[b.first_scan + k], &msg, &bytes);
      if (st != ILCC_OK) return st;
      if (L.data_offset + L.data_bytes > bytes) return fail(ILCC_IO_ERROR, "a cloud message changed between two reads of the bag");
      at = align16(at);
      if (L.data_bytes) std::memcpy(B->h_blob.p + at, msg.data() + L.data_offset, L.data_bytes);
      B->src.push_back(at);
      at += L.data_bytes;
    }
    for (const ImageSlot& slot : b.images) {
      const ilcc_image_layout& I = image_of_topic[slot.image];
      const int32_t st = read_message(images, slot.image, &msg, &bytes);
      if (st != ILCC_OK) return st;
      if (I.data_offset + (uint64_t)I.step * I.height > bytes) return fail(ILCC_IO_ERROR, "an image message changed between two reads of the bag");
      std::memcpy(B->h_raw.p + slot.raw_at, msg.data() + I.data_offset, (uint64_t)I.step * I.height);
    }
    return ILCC_OK;
  }

  // everything the device does for the batch, queued on s
  int32_t submit(Buffers* B, hipStream_t s) {
    const Batch& b = *B->batch;
    hipError_t e;
    if (b.blob_bytes && (e = hipMemcpyAsync(B->d_blob.p, B->h_blob.p, b.blob_bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e);
    B->offsets.assign(b.scans + 1, 0);
    int32_t st = ilcc_pointcloud2_unpack_batch_device(B->d_blob.p, b.blob_bytes, &cloud_of[b.first_scan], B->src.data(), b.scans, B->d_xyzi.p,
                                                      b.points, B->offsets.data(), B->unpack, s);
    if (st != ILCC_OK) return st;
    std::vector<const void*> image_ptrs;
    std::vector<uint32_t> steps;
    std::vector<int32_t> image_of_scan(b.scans, -1);
    for (const ImageSlot& slot : b.images) {
      const ilcc_image_layout& I = image_of_topic[slot.image];
      uint8_t* raw = static_cast<uint8_t*>(B->d_raw.p) + slot.raw_at;
      uint8_t* bgr = static_cast<uint8_t*>(B->d_bgr.p) + slot.bgr_at;
      if ((e = hipMemcpyAsync(raw, B->h_raw.p + slot.raw_at, (uint64_t)I.step * I.height, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e);
      st = ilcc_image_to_bgr8_device(raw, (int32_t)I.width, (int32_t)I.height, (int32_t)I.step, (int32_t)I.encoding, sample_raw ? nullptr : camera, bgr,
                                     3 * (int32_t)I.width, s);
      if (st != ILCC_OK) return st;
      for (uint32_t k = 0; k < b.scans; ++k)
        if (pair[b.first_scan + k] == (int64_t)slot.image) image_of_scan[k] = (int32_t)image_ptrs.size();
      image_ptrs.push_back(bgr);
      steps.push_back(3u * I.width);
    }
    return ilcc_colourise_batch_device(B->d_xyzi.p, B->offsets.data(), b.scans, image_ptrs.data(), steps.data(), (uint32_t)image_ptrs.size(),
                                       image_of_scan.data(), &proj, distance_valid, B->d_records.p, b.points, B->colour, s);
  }
};

// the distinct images the scans [first, first + scans) need, in the order they are first needed
void images_of(const Chain& c, uint32_t first, uint32_t scans, std::vector<uint32_t>* out) {
  out->clear();
  for (uint32_t k = 0; k < scans; ++k) {
    const int64_t j = c.pair[first + k];
    if (j >= 0 && std::find(out->begin(), out->end(), (uint32_t)j) == out->end()) out->push_back((uint32_t)j);
  }
}

int32_t all_scans(int32_t device, const char* image_bag, const char* image_topic, const char* lidar_bag, const char* lidar_topic,
                  const ilcc_camera_model* camera, const double* T, double distance_valid, const ilcc_paired_params& pp, ilcc_pair_sink sink,
                  void* user, uint32_t* n_scans, uint32_t* n_paired) {
  if (camera->width <= 0 || camera->height <= 0) return fail(ILCC_BAD_ARGUMENT, "the camera's width and height must be positive");
  Iterator cloud_it, image_it;
  int32_t st = ilcc_bag_topic_open(lidar_bag, lidar_topic, nullptr, &cloud_it.it);
  if (st != ILCC_OK) return st;
  st = ilcc_bag_topic_open(image_bag, image_topic, kImageMd5, &image_it.it);
  if (st == ILCC_BAD_ARGUMENT) {   // no sensor_msgs/Image there: say so when the topic carries the compressed type instead
    Iterator compressed;
    if (ilcc_bag_topic_open(image_bag, image_topic, kCompressedImageMd5, &compressed.it) == ILCC_OK)
      return fail(ILCC_BAD_ARGUMENT, std::string("topic ") + image_topic +
                                         " carries only sensor_msgs/CompressedImage: ilcc_bag_rgblidar_all_scans takes sensor_msgs/Image");
    return ilcc_bag_topic_open(image_bag, image_topic, kImageMd5, &compressed.it);   // the first refusal, with its text
  }
  if (st != ILCC_OK) return st;

  Chain c;
  c.clouds = cloud_it.it;
  c.images = image_it.it;
  c.camera = camera;
  c.sample_raw = pp.sample_raw != 0;
  c.distance_valid = distance_valid;
  const int32_t w = camera->width, h = camera->height;
  c.proj = ilcc_projection{{T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, {T[3], T[7], T[11]}, camera->fx, camera->cx, camera->fy, camera->cy, w, h};
  c.bgr_image_bytes = align256(3ull * (uint64_t)w * (uint64_t)h);

  // every image's header, once
  const uint64_t n_images = ilcc_bag_topic_count(image_it.it);
  uint64_t bytes = 0;
  c.image_of_topic.resize(n_images);
  std::vector<uint64_t> image_ns(n_images);
  for (uint64_t j = 0; j < n_images; ++j) {
    if ((st = read_message(image_it.it, j, &c.msg, &bytes)) != ILCC_OK) return st;
    ilcc_image_layout& I = c.image_of_topic[j];
    if ((st = ilcc_image_parse_any(c.msg.data(), bytes, &I)) != ILCC_OK) return st;
    if ((int64_t)I.width != w || (int64_t)I.height != h)
      return fail(ILCC_BAD_ARGUMENT, "image message " + std::to_string(j) + " is " + std::to_string(I.width) + " x " + std::to_string(I.height) +
                                         ", the camera " + std::to_string(w) + " x " + std::to_string(h));
    if (I.step > (uint32_t)INT32_MAX) return fail(ILCC_BAD_ARGUMENT, "image step too large");
    image_ns[j] = stamp_ns(I.stamp_sec, I.stamp_nsec);
  }

  // the selected clouds' headers, once; then the pairing
  const uint64_t count = ilcc_bag_topic_count(cloud_it.it), stride = pp.stride ? pp.stride : 1;
  for (uint64_t i = pp.first; i < count && (pp.max_scans == 0 || c.selected.size() < pp.max_scans); i += stride) c.selected.push_back(i);
  if (c.selected.empty()) return fail(ILCC_BAD_ARGUMENT, "first / stride / max_scans select no message of the topic");
  const uint32_t n_sel = (uint32_t)c.selected.size();
  c.cloud_of.resize(n_sel);
  std::vector<uint64_t> cloud_ns(n_sel);
  for (uint32_t s = 0; s < n_sel; ++s) {
    if ((st = read_message(cloud_it.it, c.selected[s], &c.msg, &bytes)) != ILCC_OK) return st;
    if ((st = ilcc_pointcloud2_parse(c.msg.data(), bytes, &c.cloud_of[s])) != ILCC_OK) return st;
    cloud_ns[s] = stamp_ns(c.cloud_of[s].stamp_sec, c.cloud_of[s].stamp_nsec);
  }
  c.pair.assign(n_sel, -1);
  c.dt.assign(n_sel, 0);
  st = ilcc_pair_by_stamp(cloud_ns.data(), n_sel, image_ns.data(), n_images, pp.max_dt_ns, c.pair.data(), c.dt.data());
  if (st != ILCC_OK) return fail(st, "pairing failed");
  // the nearest image of an unpaired scan, for its record: the pairing again without a limit
  std::vector<int64_t> nearest(n_sel, -1), unused(n_sel, 0);
  (void)ilcc_pair_by_stamp(cloud_ns.data(), n_sel, image_ns.data(), n_images, UINT64_MAX, nearest.data(), unused.data());
  *n_scans = n_sel;
  *n_paired = (uint32_t)std::count_if(c.pair.begin(), c.pair.end(), [](int64_t j) { return j >= 0; });

  // the batches, by the two budgets
  const uint64_t staging = pp.staging_bytes ? pp.staging_bytes : kDefaultStagingBytes, image_budget = pp.image_bytes ? pp.image_bytes : kDefaultImageBytes;
  const auto raw_bytes = [&](uint32_t j) { return align256((uint64_t)c.image_of_topic[j].step * c.image_of_topic[j].height); };
  std::vector<uint32_t> needed;
  for (uint32_t s = 0; s < n_sel;) {
    Batch b;
    b.first_scan = s;
    uint64_t image_cost = 0;
    while (s < n_sel) {
      const ilcc_pointcloud2_layout& L = c.cloud_of[s];
      const uint64_t pts = (uint64_t)L.height * L.width, at = align16(b.blob_bytes);
      uint64_t extra = 0;
      const int64_t j = c.pair[s];
      images_of(c, b.first_scan, b.scans, &needed);
      if (j >= 0 && std::find(needed.begin(), needed.end(), (uint32_t)j) == needed.end()) extra = raw_bytes((uint32_t)j) + c.bgr_image_bytes;
      if (L.data_bytes > staging) return fail(ILCC_CAPACITY, "a scan's data[] is larger than staging_bytes");
      if (extra > image_budget) return fail(ILCC_CAPACITY, "an image (raw + B,G,R) is larger than image_bytes");
      if (b.points + pts > 0xFFFFFFFEull) {
        if (b.scans == 0) return fail(ILCC_BAD_ARGUMENT, "cloud of more than 2^32 - 2 points");
        break;
      }
      if (b.scans > 0 && (at + L.data_bytes > staging || image_cost + extra > image_budget)) break;
      b.blob_bytes = at + L.data_bytes;
      b.points += pts;
      image_cost += extra;
      ++b.scans;
      ++s;
    }
    images_of(c, b.first_scan, b.scans, &needed);
    for (uint32_t j : needed) {
      b.images.push_back(ImageSlot{j, b.raw_bytes, b.bgr_bytes});
      b.raw_bytes += raw_bytes(j);
      b.bgr_bytes += c.bgr_image_bytes;
    }
    c.batches.push_back(std::move(b));
  }
  Batch largest;
  for (const Batch& b : c.batches) {
    largest.scans = std::max(largest.scans, b.scans);
    largest.blob_bytes = std::max(largest.blob_bytes, b.blob_bytes);
    largest.points = std::max(largest.points, b.points);
    largest.raw_bytes = std::max(largest.raw_bytes, b.raw_bytes);
    largest.bgr_bytes = std::max(largest.bgr_bytes, b.bgr_bytes);
  }

  // one set of allocations for the whole call
  if ((st = select_device(device)) != ILCC_OK) return st;
  hipError_t e;
  Stream stream;
  if ((e = hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking)) != hipSuccess) return hip_fail(e);
  Buffers B[2];
  const int sets = c.batches.size() > 1 ? 2 : 1;
  for (int k = 0; k < sets; ++k) {
    Buffers& b = B[k];
    const uint64_t records = 16 * std::max<uint64_t>(largest.points, 1);
    if ((e = hipHostMalloc((void**)&b.h_blob.p, std::max<uint64_t>(largest.blob_bytes, 16), hipHostMallocDefault)) != hipSuccess ||
        (e = hipHostMalloc((void**)&b.h_raw.p, std::max<uint64_t>(largest.raw_bytes, 16), hipHostMallocDefault)) != hipSuccess ||
        (e = hipHostMalloc((void**)&b.h_records.p, records, hipHostMallocDefault)) != hipSuccess ||
        (e = hipMalloc(&b.d_blob.p, std::max<uint64_t>(largest.blob_bytes, 16))) != hipSuccess || (e = hipMalloc(&b.d_xyzi.p, records)) != hipSuccess ||
        (e = hipMalloc(&b.d_raw.p, std::max<uint64_t>(largest.raw_bytes, 16))) != hipSuccess ||
        (e = hipMalloc(&b.d_bgr.p, std::max<uint64_t>(largest.bgr_bytes, 16))) != hipSuccess || (e = hipMalloc(&b.d_records.p, records)) != hipSuccess)
      return hip_fail(e);
    if (!(b.unpack = ilcc_unpack_plan_create(largest.scans))) return ILCC_HIP_ERROR;
    if (!(b.colour = ilcc_colourise_plan_create(largest.scans, std::max<uint64_t>(largest.points, 1)))) return ILCC_HIP_ERROR;
  }
  InFlight flying;   // declared behind the buffers: its destructor runs before theirs
  flying.s = stream.s;

  // the batches: while the device works on batch k the host reads, inflates and stages batch k + 1
  if ((st = c.stage(&B[0], c.batches[0])) != ILCC_OK || (st = c.submit(&B[0], stream.s)) != ILCC_OK) return st;
  for (size_t k = 0; k < c.batches.size(); ++k) {
    Buffers& now = B[k & 1];
    Buffers& next = B[(k + 1) & 1];   // its previous batch has been finished, copied back and handed to the sink
    const bool more = k + 1 < c.batches.size();
    int32_t st_next = more ? c.stage(&next, c.batches[k + 1]) : ILCC_OK;
    const Batch& b = *now.batch;
    now.out_offsets.assign(b.scans + 1, 0);
    if ((st = ilcc_colourise_plan_finish(now.colour, now.out_offsets.data())) != ILCC_OK) return st;
    if (st_next != ILCC_OK) return st_next;
    if (more && (st = c.submit(&next, stream.s)) != ILCC_OK) return st;   // the device goes on while the host copies back and sinks
    const uint64_t total = now.out_offsets[b.scans];
    if (total && (e = hipMemcpy(now.h_records.p, now.d_records.p, 16 * total, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e);
    for (uint32_t s = 0; s < b.scans; ++s) {
      const uint32_t g = b.first_scan + s;
      ilcc_pair_record r;
      std::memset(&r, 0, sizeof(r));
      r.message = (uint32_t)c.selected[g];
      r.stamp_sec = c.cloud_of[g].stamp_sec;
      r.stamp_nsec = c.cloud_of[g].stamp_nsec;
      r.image_message = (int32_t)c.pair[g];
      if (nearest[g] >= 0) {
        r.image_stamp_sec = c.image_of_topic[nearest[g]].stamp_sec;
        r.image_stamp_nsec = c.image_of_topic[nearest[g]].stamp_nsec;
      }
      r.dt_ns = c.dt[g];
      r.n_points = (uint64_t)c.cloud_of[g].height * c.cloud_of[g].width;
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
  pp->staging_bytes = kDefaultStagingBytes;
  pp->image_bytes = kDefaultImageBytes;
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
