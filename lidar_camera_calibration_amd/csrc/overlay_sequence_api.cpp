// overlay_sequence_api.cpp -- ilcc_bag_pcd2image_all_pairs (include/ilcc_overlay_sequence.h): every selected scan of a recording
// drawn on the image whose header stamp is nearest to its own, and written as a JPEG file's bytes.  The layers below do the work:
// the topic iterator (bag_reader.cpp), the pairing (paired_host.cpp), K0b (k0b_unpack_batch.hip), K11c (k11_camera_image.hip), K12b
// (k12b_overlay_batch.hip), K14b (k14b_jpeg_write_batch.hip), K17 (k17_jpeg_huffman_enc.hip), the headers and the host encoder
// (jpeg_entropy_enc.cpp), the bytes of a paired scan (overlay_sequence_host.cpp).  This file owns the batching, which is
// paired_api.cpp's with a third budget: it reads every header once, cuts the selected scans into batches BEFORE anything is
// allocated, and runs the batches through two sets of buffers.  An unpaired scan is never staged: it costs a record.  The part
// "rows and scans of a batch -> the files' bytes" restates jpeg_write_sequence_api.cpp's for three components and a sink instead
// of files; that file is left as it is.  Failures below are reported through ilcc_last_error(NULL).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "host_util.h"
#include "ilcc_jpeg_write.h"
#include "ilcc_jpeg_write_sequence.h"
#include "ilcc_overlay_sequence.h"
#include "ilcc_paired.h"

using namespace ilcc;

namespace {

constexpr const char* kImageMd5 = "060021388200f6f0f447d0fcd9c64743";
constexpr const char* kCompressedImageMd5 = "8f7a12909da2c9d3332d540a0977563f";
constexpr uint64_t kHeaderRoom = 1024;   // above the 629 bytes the headers can take

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
  uint32_t first_scan = 0, scans = 0;   // among the selected scans, unpaired ones included
  std::vector<uint32_t> members;        // the paired ones, as indices among the selected scans: what the device sees
  uint64_t blob_bytes = 0, points = 0, raw_bytes = 0, bgr_bytes = 0;
  std::vector<ImageSlot> images;
};

// what one picture takes on the device, every part a multiple of 256 (overlay_sequence_host.cpp sums the same parts)
struct Sizes {
  uint64_t canvas, owner, coef, fdct, out_per_image;
};

// one of the two sets of buffers
struct Buffers {
  Pinned h_blob, h_raw, h_back, h_pixels, h_coef;   // h_back: [ rows | scans ]
  DeviceBuffer d_blob, d_xyzi, d_raw, d_bgr, d_pictures;   // d_pictures: [ canvases | owner | coefficients | K14b's planes | scans | rows | K17's scratch ]
  uint64_t owner_at = 0, coef_at = 0, fdct_at = 0, out_at = 0, rows_at = 0, k17_at = 0, k17_bytes = 0, back_rows = 0;
  ilcc_unpack_plan* unpack = nullptr;
  ilcc_overlay_plan* overlay = nullptr;
  std::vector<uint64_t> src, offsets;
  std::vector<ilcc_pointcloud2_layout> layouts;
  std::vector<uint32_t> n_drawn;
  const Batch* batch = nullptr;
  ~Buffers() {
    ilcc_unpack_plan_destroy(unpack);
    ilcc_overlay_plan_destroy(overlay);
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
  ilcc_projection proj{};
  double distance_valid = 0;
  uint64_t bgr_image_bytes = 0;
  ilcc_jpeg_info info{};
  Sizes S{};
  uint32_t route = 0;
  bool keep_pixels = false;

  // host only: the batch's messages into the page-locked buffers
  int32_t stage(Buffers* B, const Batch& b) {
    B->batch = &b;
    B->src.clear();
    B->layouts.clear();
    uint64_t at = 0, bytes = 0;
    for (uint32_t g : b.members) {
      const ilcc_pointcloud2_layout& L = cloud_of[g];
      const int32_t st = read_message(clouds, selected[g], &msg, &bytes);
      if (st != ILCC_OK) return st;
      if (L.data_offset + L.data_bytes > bytes) return fail(ILCC_IO_ERROR, "a cloud message changed between two reads of the bag");
      at = align16(at);
      if (L.data_bytes) std::memcpy(B->h_blob.p + at, msg.data() + L.data_offset, L.data_bytes);
      B->src.push_back(at);
      B->layouts.push_back(L);
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

  // everything the device does for the batch up to the rows, queued on s
  int32_t submit(Buffers* B, hipStream_t s) {
    const Batch& b = *B->batch;
    const uint32_t m = (uint32_t)b.members.size();
    if (m == 0) return ILCC_OK;
    hipError_t e;
    if (b.blob_bytes && (e = hipMemcpyAsync(B->d_blob.p, B->h_blob.p, b.blob_bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e);
    B->offsets.assign(m + 1, 0);
    int32_t st = ilcc_pointcloud2_unpack_batch_device(B->d_blob.p, b.blob_bytes, B->layouts.data(), B->src.data(), m, B->d_xyzi.p, b.points,
                                                      B->offsets.data(), B->unpack, s);
    if (st != ILCC_OK) return st;
    std::vector<const void*> image_ptrs;
    std::vector<uint32_t> steps;
    std::vector<int32_t> image_of_scan(m, -1);
    const int32_t w = proj.width;
    for (const ImageSlot& slot : b.images) {
      const ilcc_image_layout& I = image_of_topic[slot.image];
      uint8_t* raw = static_cast<uint8_t*>(B->d_raw.p) + slot.raw_at;
      uint8_t* bgr = static_cast<uint8_t*>(B->d_bgr.p) + slot.bgr_at;
      if ((e = hipMemcpyAsync(raw, B->h_raw.p + slot.raw_at, (uint64_t)I.step * I.height, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e);
      st = ilcc_image_to_bgr8_device(raw, (int32_t)I.width, (int32_t)I.height, (int32_t)I.step, (int32_t)I.encoding, camera, bgr, 3 * (int32_t)I.width, s);
      if (st != ILCC_OK) return st;
      for (uint32_t k = 0; k < m; ++k)
        if (pair[b.members[k]] == (int64_t)slot.image) image_of_scan[k] = (int32_t)image_ptrs.size();
      image_ptrs.push_back(bgr);
      steps.push_back(3u * I.width);
    }
    uint8_t* base = static_cast<uint8_t*>(B->d_pictures.p);
    ilcc_overlay_batch_job oj{};
    oj.d_xyzi = B->d_xyzi.p;
    oj.offsets = B->offsets.data();
    oj.d_images_bgr = image_ptrs.data();
    oj.image_steps = steps.data();
    oj.image_of_scan = image_of_scan.data();
    oj.cam = &proj;
    oj.d_canvas = base;
    oj.d_scratch = base + B->owner_at;
    oj.plan = B->overlay;
    oj.hip_stream = s;
    oj.canvas_pitch = S.canvas;
    oj.scratch_bytes = S.owner * m;
    oj.distance_valid = distance_valid;
    oj.inten_low = 0.0;    // pcd2image.cpp fixes the colour range
    oj.inten_high = 60.0;
    oj.n_scans = m;
    oj.n_images = (uint32_t)image_ptrs.size();
    oj.canvas_stride = 3 * w;
    if ((st = ilcc_overlay_batch_device(&oj)) != ILCC_OK) return st;
    ilcc_jpeg_fdct_batch_job fj{};
    fj.layout = &info;
    fj.d_src = base;
    fj.image_pitch = S.canvas;
    fj.src_stride = 3 * w;
    fj.encoding = ILCC_ENCODING_BGR8;
    fj.d_coef = reinterpret_cast<int16_t*>(base + B->coef_at);
    fj.coef_pitch = S.coef / sizeof(int16_t);
    fj.d_scratch = base + B->fdct_at;
    fj.scratch_bytes = S.fdct * m;
    fj.n_images = m;
    fj.hip_stream = s;
    if ((st = ilcc_jpeg_fdct_batch_device(&fj)) != ILCC_OK) return st;
    if (route == 0) {
      ilcc_jpeg_huffman_encode_job hj{};
      hj.layout = &info;
      hj.d_coef = fj.d_coef;
      hj.coef_pitch = fj.coef_pitch;
      hj.d_out = base + B->out_at;
      hj.out_cap = S.out_per_image * m;
      hj.d_rows = reinterpret_cast<ilcc_jpeg_encode_row*>(base + B->rows_at);
      hj.d_scratch = base + B->k17_at;
      hj.scratch_bytes = B->k17_bytes;
      hj.n_images = m;
      hj.hip_stream = s;
      if ((st = ilcc_jpeg_huffman_encode_batch_device(&hj)) != ILCC_OK) return st;
      if ((e = hipMemcpyAsync(B->h_back.p, hj.d_rows, sizeof(ilcc_jpeg_encode_row) * m, hipMemcpyDeviceToHost, s)) != hipSuccess) return hip_fail(e);
    }
    return ILCC_OK;
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

int32_t all_pairs(int32_t device, const char* image_bag, const char* image_topic, const char* lidar_bag, const char* lidar_topic,
                  const ilcc_camera_model* camera, const double* T, double distance_valid, int32_t quality, const ilcc_overlay_sequence_params& sp,
                  ilcc_overlay_sink sink, void* user, uint32_t* n_scans, uint32_t* n_paired) {
  if (camera->width <= 0 || camera->height <= 0) return fail(ILCC_BAD_ARGUMENT, "the camera's width and height must be positive");
  Iterator cloud_it, image_it;
  int32_t st = ilcc_bag_topic_open(lidar_bag, lidar_topic, nullptr, &cloud_it.it);
  if (st != ILCC_OK) return st;
  st = ilcc_bag_topic_open(image_bag, image_topic, kImageMd5, &image_it.it);
  if (st == ILCC_BAD_ARGUMENT) {   // no sensor_msgs/Image there: say so when the topic carries the compressed type instead
    Iterator compressed;
    if (ilcc_bag_topic_open(image_bag, image_topic, kCompressedImageMd5, &compressed.it) == ILCC_OK)
      return fail(ILCC_BAD_ARGUMENT, std::string("topic ") + image_topic +
                                         " carries only sensor_msgs/CompressedImage: ilcc_bag_pcd2image_all_pairs takes sensor_msgs/Image");
    return ilcc_bag_topic_open(image_bag, image_topic, kImageMd5, &compressed.it);   // the first refusal, with its text
  }
  if (st != ILCC_OK) return st;

  Chain c;
  c.clouds = cloud_it.it;
  c.images = image_it.it;
  c.camera = camera;
  c.distance_valid = distance_valid;
  c.route = sp.route;
  c.keep_pixels = sp.keep_pixels != 0;
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

  // the file every picture becomes: 3 components, 4:2:0, no restart markers, as ilcc_jpeg_write_file writes it
  if ((st = ilcc_jpeg_write_info(w, h, 3, 2, 2, quality, 0, &c.info)) != ILCC_OK) return st;
  const uint64_t pixels = (uint64_t)w * (uint64_t)h;
  c.S.canvas = align256(3 * pixels);
  c.S.owner = align256(4 * pixels);   // a multiple of 16: K12b's plane pitch is ilcc_overlay_batch_scratch_bytes(w, h, 1) <= this
  c.S.coef = align256(c.info.coef_count * sizeof(int16_t));
  c.S.fdct = align256(ilcc_jpeg_fdct_scratch_bytes(&c.info));
  c.S.out_per_image = align16(sp.out_bytes_per_image ? sp.out_bytes_per_image : pixels);
  const uint64_t per_scan = ilcc_overlay_sequence_bytes(w, h, sp.out_bytes_per_image);
  if (per_scan == 0) return fail(ILCC_BAD_ARGUMENT, "image too large for K17, or out_bytes_per_image of 2^40 or more");

  // the selected clouds' headers, once; then the pairing
  const uint64_t count = ilcc_bag_topic_count(cloud_it.it), stride = sp.stride ? sp.stride : 1;
  for (uint64_t i = sp.first; i < count && (sp.max_scans == 0 || c.selected.size() < sp.max_scans); i += stride) c.selected.push_back(i);
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
  st = ilcc_pair_by_stamp(cloud_ns.data(), n_sel, image_ns.data(), n_images, sp.max_dt_ns, c.pair.data(), c.dt.data());
  if (st != ILCC_OK) return fail(st, "pairing failed");
  // the nearest image of an unpaired scan, for its record: the pairing again without a limit
  std::vector<int64_t> nearest(n_sel, -1), unused(n_sel, 0);
  (void)ilcc_pair_by_stamp(cloud_ns.data(), n_sel, image_ns.data(), n_images, UINT64_MAX, nearest.data(), unused.data());
  *n_scans = n_sel;
  *n_paired = (uint32_t)std::count_if(c.pair.begin(), c.pair.end(), [](int64_t j) { return j >= 0; });

  // the batches, by the three budgets
  const uint64_t staging = sp.staging_bytes ? sp.staging_bytes : 256ull << 20, image_budget = sp.image_bytes ? sp.image_bytes : 512ull << 20;
  const uint64_t device_budget = sp.device_bytes ? sp.device_bytes : 1ull << 30;
  if (per_scan > device_budget) return fail(ILCC_CAPACITY, "one paired scan (" + std::to_string(per_scan) + " device bytes) is above device_bytes");
  const auto raw_bytes = [&](uint32_t j) { return align256((uint64_t)c.image_of_topic[j].step * c.image_of_topic[j].height); };
  std::vector<uint32_t> needed;
  for (uint32_t s = 0; s < n_sel;) {
    Batch b;
    b.first_scan = s;
    uint64_t image_cost = 0, counted = 0;   // counted: the data[] of every scan of the batch, as ilcc_bag_rgblidar_all_scans counts it
    while (s < n_sel) {
      const int64_t j = c.pair[s];
      const ilcc_pointcloud2_layout& L = c.cloud_of[s];
      const uint64_t pts = (uint64_t)L.height * L.width, counted_at = align16(counted);
      if (L.data_bytes > staging) return fail(ILCC_CAPACITY, "a scan's data[] is larger than staging_bytes");
      uint64_t extra = 0;
      images_of(c, b.first_scan, b.scans, &needed);
      if (j >= 0 && std::find(needed.begin(), needed.end(), (uint32_t)j) == needed.end()) extra = raw_bytes((uint32_t)j) + c.bgr_image_bytes;
      if (extra > image_budget) return fail(ILCC_CAPACITY, "an image (raw + B,G,R) is larger than image_bytes");
      if (j >= 0 && b.points + pts > 0xFFFFFFFEull) {
        if (b.members.empty()) return fail(ILCC_BAD_ARGUMENT, "cloud of more than 2^32 - 2 points");
        break;
      }
      if (b.scans > 0 && (counted_at + L.data_bytes > staging || image_cost + extra > image_budget ||
                          (j >= 0 && ((b.members.size() + 1) * per_scan > device_budget || b.members.size() >= 65535u))))
        break;
      counted = counted_at + L.data_bytes;
      if (j >= 0) {   // an unpaired scan is counted like any other, but never staged: it becomes a record, nothing on the device
        b.blob_bytes = align16(b.blob_bytes) + L.data_bytes;
        b.points += pts;
        image_cost += extra;
        b.members.push_back(s);
      }
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
  uint32_t members_max = 0;
  for (const Batch& b : c.batches) {
    members_max = std::max<uint32_t>(members_max, (uint32_t)b.members.size());
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
  const uint64_t mm = std::max<uint32_t>(members_max, 1), out_cap_max = c.S.out_per_image * mm;
  const uint64_t coef_bytes = c.info.coef_count * sizeof(int16_t);
  for (int k = 0; k < sets && members_max; ++k) {
    Buffers& b = B[k];
    b.owner_at = c.S.canvas * mm;
    b.coef_at = b.owner_at + c.S.owner * mm;
    b.fdct_at = b.coef_at + c.S.coef * mm;
    b.out_at = b.fdct_at + c.S.fdct * mm;
    b.rows_at = b.out_at + align256(out_cap_max);
    b.k17_at = b.rows_at + align256(sizeof(ilcc_jpeg_encode_row) * mm);
    b.k17_bytes = ilcc_jpeg_huffman_encode_scratch_bytes(&c.info, (uint32_t)mm, out_cap_max);
    if (b.k17_bytes == 0) return fail(ILCC_BAD_ARGUMENT, "a batch's pictures are too large for K17");
    b.back_rows = align256(sizeof(ilcc_jpeg_encode_row) * mm);
    const uint64_t points16 = 16 * std::max<uint64_t>(largest.points, 1);
    if ((e = hipHostMalloc((void**)&b.h_blob.p, std::max<uint64_t>(largest.blob_bytes, 16), hipHostMallocDefault)) != hipSuccess ||
        (e = hipHostMalloc((void**)&b.h_raw.p, std::max<uint64_t>(largest.raw_bytes, 16), hipHostMallocDefault)) != hipSuccess ||
        (e = hipHostMalloc((void**)&b.h_back.p, b.back_rows + out_cap_max, hipHostMallocDefault)) != hipSuccess ||
        (e = hipHostMalloc((void**)&b.h_coef.p, coef_bytes, hipHostMallocDefault)) != hipSuccess ||
        (c.keep_pixels && (e = hipHostMalloc((void**)&b.h_pixels.p, c.S.canvas * mm, hipHostMallocDefault)) != hipSuccess) ||
        (e = hipMalloc(&b.d_blob.p, std::max<uint64_t>(largest.blob_bytes, 16))) != hipSuccess || (e = hipMalloc(&b.d_xyzi.p, points16)) != hipSuccess ||
        (e = hipMalloc(&b.d_raw.p, std::max<uint64_t>(largest.raw_bytes, 16))) != hipSuccess ||
        (e = hipMalloc(&b.d_bgr.p, std::max<uint64_t>(largest.bgr_bytes, 16))) != hipSuccess || (e = hipMalloc(&b.d_pictures.p, b.k17_at + b.k17_bytes)) != hipSuccess)
      return hip_fail(e);
    if (!(b.unpack = ilcc_unpack_plan_create((uint32_t)mm))) return ILCC_HIP_ERROR;
    if (!(b.overlay = ilcc_overlay_plan_create((uint32_t)mm, std::max<uint64_t>(largest.points, 1)))) return ILCC_HIP_ERROR;
  }
  InFlight flying;   // declared behind the buffers: its destructor runs before theirs
  flying.s = stream.s;

  uint8_t headers[kHeaderRoom];
  uint64_t header_bytes = 0;
  if ((st = ilcc_jpeg_write_headers(&c.info, headers, sizeof(headers), &header_bytes)) != ILCC_OK) return st;
  std::vector<std::vector<uint8_t>> files(mm);   // of the batch being handed to the sink
  std::vector<uint32_t> route_of(mm);

  // picture k of the batch in `now` by the host encoder: its coefficients to the host, ilcc_jpeg_entropy_encode, the file's bytes
  auto host_encode = [&](Buffers& now, uint32_t k) -> int32_t {
    const Batch& b = *now.batch;
    hipError_t err = hipMemcpyAsync(now.h_coef.p, static_cast<uint8_t*>(now.d_pictures.p) + now.coef_at + c.S.coef * k, coef_bytes, hipMemcpyDeviceToHost, stream.s);
    if (err == hipSuccess) err = hipStreamSynchronize(stream.s);
    if (err != hipSuccess) return hip_fail(err);
    const uint64_t bound = ilcc_jpeg_file_bound(&c.info);
    uint64_t room = std::min<uint64_t>(1024 + c.info.coef_count, bound), n = 0;   // a byte per coefficient holds any file an image compresses into
    for (;;) {
      files[k].resize(room);
      const int32_t s = ilcc_jpeg_entropy_encode(&c.info, reinterpret_cast<const int16_t*>(now.h_coef.p), files[k].data(), room, &n);
      if (s == ILCC_CAPACITY && room < bound) {
        room = bound;
        continue;
      }
      if (s != ILCC_OK) return fail(s, "cloud message " + std::to_string(c.selected[b.members[k]]) + ": " + ilcc_last_error(nullptr));
      break;
    }
    files[k].resize(n);
    route_of[k] = 1;
    return ILCC_OK;
  };

  // the batches: while the device works on batch k the host reads and stages batch k + 1; while it works on k + 1 the host sinks k
  if ((st = c.stage(&B[0], c.batches[0])) != ILCC_OK || (st = c.submit(&B[0], stream.s)) != ILCC_OK) return st;
  for (size_t k = 0; k < c.batches.size(); ++k) {
    Buffers& now = B[k & 1];
    Buffers& next = B[(k + 1) & 1];   // its previous batch has been finished, copied back and handed to the sink
    const bool more = k + 1 < c.batches.size();
    const int32_t st_next = more ? c.stage(&next, c.batches[k + 1]) : ILCC_OK;
    const Batch& b = *now.batch;
    const uint32_t m = (uint32_t)b.members.size();
    if (m) {
      now.n_drawn.assign(m, 0);
      if ((st = ilcc_overlay_plan_finish(now.overlay, now.n_drawn.data())) != ILCC_OK) return st;
      if ((e = hipStreamSynchronize(stream.s)) != hipSuccess) return hip_fail(e);   // only this batch is on the stream: the rows are here
      uint8_t* base = static_cast<uint8_t*>(now.d_pictures.p);
      const auto* rows = reinterpret_cast<const ilcc_jpeg_encode_row*>(now.h_back.p);
      const uint8_t* payload = now.h_back.p + now.back_rows;
      if (c.keep_pixels && (e = hipMemcpyAsync(now.h_pixels.p, base, c.S.canvas * m, hipMemcpyDeviceToHost, stream.s)) != hipSuccess) return hip_fail(e);
      if (c.route == 0) {
        uint64_t span = 0;
        for (uint32_t i = 0; i < m; ++i)
          if (rows[i].status == 0) span = std::max(span, rows[i].offset + rows[i].bytes);
        if (span > c.S.out_per_image * m) return fail(ILCC_HIP_ERROR, "internal error: K17 placed a scan past its output");
        if (span && (e = hipMemcpyAsync(now.h_back.p + now.back_rows, base + now.out_at, span, hipMemcpyDeviceToHost, stream.s)) != hipSuccess) return hip_fail(e);
      }
      if ((e = hipStreamSynchronize(stream.s)) != hipSuccess) return hip_fail(e);
      for (uint32_t i = 0; i < m; ++i) {
        if (c.route == 0 && rows[i].status == 0) {   // headers + scan + EOI
          std::vector<uint8_t>& f = files[i];
          f.resize(header_bytes + rows[i].bytes + 2);
          std::memcpy(f.data(), headers, header_bytes);
          std::memcpy(f.data() + header_bytes, payload + rows[i].offset, rows[i].bytes);
          f[header_bytes + rows[i].bytes] = 0xFF;
          f[header_bytes + rows[i].bytes + 1] = 0xD9;
          route_of[i] = 0;
          continue;
        }
        // route 1, or what K17 did not place: a picture without room is finished by the host encoder; a range refusal is its to word
        if ((st = host_encode(now, i)) != ILCC_OK) return st;
        if (c.route == 0 && (rows[i].status & (ILCC_JPEG_ENCODE_DC_RANGE | ILCC_JPEG_ENCODE_AC_RANGE)))
          return fail(ILCC_HIP_ERROR, "cloud message " + std::to_string(c.selected[b.members[i]]) + ": internal error: K17 refused coefficients (status " +
                                          std::to_string(rows[i].status) + ") that the host encoder accepts");
      }
    }
    if (st_next != ILCC_OK) return st_next;
    if (more && (st = c.submit(&next, stream.s)) != ILCC_OK) return st;   // the device goes on while the host sinks
    uint32_t member = 0;
    for (uint32_t s = 0; s < b.scans; ++s) {
      const uint32_t g = b.first_scan + s;
      ilcc_overlay_record r;
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
      const uint8_t* jpeg = nullptr;
      const uint8_t* bgr = nullptr;
      if (c.pair[g] >= 0) {
        r.n_drawn = now.n_drawn[member];
        r.route = route_of[member];
        r.file_bytes = files[member].size();
        jpeg = files[member].data();
        if (c.keep_pixels) bgr = now.h_pixels.p + c.S.canvas * member;
        ++member;
      }
      if (sink && sink(user, &r, jpeg, r.file_bytes, bgr) != 0) return fail(ILCC_IO_ERROR, "the sink refused scan " + std::to_string(g));
    }
  }
  return ILCC_OK;
}

}  // namespace

extern "C" int32_t ilcc_bag_pcd2image_all_pairs(int32_t device, const char* image_bag, const char* image_topic, const char* lidar_bag,
                                                const char* lidar_topic, const ilcc_camera_model* camera, const double T_lidar2cam[16],
                                                double distance_valid, int32_t quality, const ilcc_overlay_sequence_params* sp, ilcc_overlay_sink sink,
                                                void* user, uint32_t* n_scans, uint32_t* n_paired) {
  if (!image_bag || !image_topic || !lidar_bag || !lidar_topic || !camera || !T_lidar2cam || !n_scans || !n_paired)
    return fail(ILCC_BAD_ARGUMENT, "ilcc_bag_pcd2image_all_pairs: null argument");
  *n_scans = *n_paired = 0;
  ilcc_overlay_sequence_params defaults;
  ilcc_default_overlay_sequence_params(&defaults);
  if (sp && sp->route > 1) return fail(ILCC_BAD_ARGUMENT, "ilcc_bag_pcd2image_all_pairs: route must be 0, K17, or 1, the host encoder");
  try {   // no exception crosses the C-ABI
    return all_pairs(device, image_bag, image_topic, lidar_bag, lidar_topic, camera, T_lidar2cam, distance_valid, quality, sp ? *sp : defaults, sink, user,
                     n_scans, n_paired);
  } catch (const std::bad_alloc&) {
    return fail(ILCC_IO_ERROR, "out of memory");
  } catch (...) {
    return fail(ILCC_IO_ERROR, "overlay sequence: unknown failure");
  }
}
