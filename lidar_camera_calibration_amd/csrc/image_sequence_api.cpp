// image_sequence_api.cpp -- ilcc_bag_corners_all_images (include/ilcc_image_sequence.h): every image of a bag topic through K11 and
// K10b, structure recovery per image, then ilcc_fuse_image_corners.  The layers below do the work: the topic iterator
// (bag_reader.cpp), the Image parser and K11 (camera_image_host.cpp, k11_camera_image.hip), K10b (k10b_image_corners_batch.hip),
// ilcc_chessboard_from_corners (image_corners_host.cpp) or K18 (structure_route.h), the cut and the fusion (image_sequence_host.cpp).  This file owns the
// batching: the two sets of buffers, and the order of the calls that lets a host thread recover batch k's boards while the
// device works on batch k + 1.  The guards, the selection, "message i in a vector" and the image-topic open are host_util.h's.
// Failures below are reported through ilcc_last_error(NULL).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "host_util.h"
#include "ilcc_image_sequence.h"
#include "ilcc_sequence.h"
#include "structure_route.h"

using namespace ilcc;

namespace {

constexpr uint64_t kDefaultStagingBytes = 256ull << 20, kDefaultDeviceBytes = 512ull << 20;
constexpr int32_t kFirstCapacity = 1024;   // corners per image; a batch with a fuller image runs again with room for it

// one of the two sets of buffers
struct BatchBuffers {
  uint8_t* h_blob = nullptr;   // page-locked
  DeviceBuffer d_blob, d_mono;
  ilcc_image_corner_plan* plan = nullptr;
  std::vector<ilcc_image_corner> corners;
  std::vector<int32_t> n_corners;
  int32_t capacity = 0;
  uint32_t first = 0, count = 0;   // the batch it carries, among the selected images
  ~BatchBuffers() {
    ilcc_image_corner_plan_destroy(plan);
    if (h_blob) (void)hipHostFree(h_blob);
  }
};

// the host thread that recovers a batch's boards; joined whatever makes the call end
struct Worker {
  std::thread t;
  int32_t status = ILCC_OK;
  std::string error;
  double ms = 0;
  void join() {
    if (t.joinable()) t.join();
  }
  ~Worker() { join(); }
};

std::string message_name(uint64_t message) { return "message " + std::to_string(message); }

void recover(const BatchBuffers* B, int32_t board_w, int32_t board_h, ilcc_image_record* records, Worker* w) {
  const auto t0 = std::chrono::steady_clock::now();
  try {
    std::vector<int32_t> idx((size_t)board_w * board_h);
    for (uint32_t m = 0; m < B->count; ++m) {
      ilcc_image_record& r = records[B->first + m];
      const ilcc_image_corner* c = B->corners.data() + (size_t)m * B->capacity;
      r.n_corners = B->n_corners[m];
      int32_t rows = 0, cols = 0;
      r.status = ilcc_chessboard_from_corners(c, r.n_corners, board_w, board_h, &rows, &cols, idx.data());
      if (r.status == ILCC_OK) {
        r.rows = rows;
        r.cols = cols;
        for (size_t i = 0; i < idx.size(); ++i) {
          r.xy[2 * i] = c[idx[i]].u;
          r.xy[2 * i + 1] = c[idx[i]].v;
        }
      } else if (r.status != ILCC_BOARD_NOT_FOUND && r.status != ILCC_AMBIGUOUS) {
        w->status = r.status;
        w->error = ilcc_last_error(nullptr);   // this thread's text
        break;
      }
    }
  } catch (...) {
    w->status = ILCC_IO_ERROR;
    w->error = "out of memory in structure recovery";
  }
  w->ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int32_t all_images(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera, int32_t board_w, int32_t board_h,
                   const ilcc_image_sequence_params& sp, ilcc_image_sequence_result* out, ilcc_image_record* per_image_out, uint32_t cap) {
  Iterator iter;
  int32_t st = open_image_topic(bag_path, topic, "ilcc_bag_corners_all_images", ", ilcc_bag_corners_all_compressed_images (ilcc_jpeg_sequence.h) takes this topic",
                                &iter.it);
  if (st != ILCC_OK) return st;
  std::vector<uint64_t> selected;
  if ((st = select_messages(iter.it, sp.first, sp.stride, sp.max_images, "max_images", &selected)) != ILCC_OK) return st;
  const uint32_t n_sel = (uint32_t)selected.size();
  out->n_images = (int32_t)n_sel;
  if (cap < n_sel && (per_image_out || cap)) return fail(ILCC_CAPACITY, "per_image_out holds fewer records than images were selected");

  // the first selected image decides size and encoding
  std::vector<uint8_t> msg;
  auto read = [&](uint32_t k, ilcc_image_layout* L) -> int32_t {
    uint64_t bytes = 0;
    int32_t s = read_message(iter.it, selected[k], &msg, &bytes);
    if (s != ILCC_OK) return s;
    if ((s = ilcc_image_parse_any(msg.data(), bytes, L)) != ILCC_OK) return fail(s, message_name(selected[k]) + ": " + ilcc_last_error(nullptr));
    return ILCC_OK;
  };
  ilcc_image_layout first;
  if ((st = read(0, &first)) != ILCC_OK) return st;
  if (first.width > 65536u || first.height > 65536u || first.step > (uint32_t)INT32_MAX)
    return fail(ILCC_BAD_ARGUMENT, message_name(selected[0]) + ": image larger than 65536 pixels a side");
  const int32_t w = (int32_t)first.width, h = (int32_t)first.height;
  if (camera && (camera->width != w || camera->height != h))
    return fail(ILCC_BAD_ARGUMENT, message_name(selected[0]) + ": the camera's width / height differ from the image's");
  const uint64_t scratch = ilcc_image_corner_scratch_bytes(w, h);
  if (!scratch)
    return fail(ILCC_BAD_ARGUMENT, message_name(selected[0]) + ": image " + std::to_string(w) + " x " + std::to_string(h) + " is smaller than 34 px a side");
  const uint64_t mono_pitch = align256((uint64_t)w * h), per_image = mono_pitch + scratch;

  // the batches, cut from the messages' lengths before anything is allocated
  std::vector<uint64_t> raw(n_sel);
  for (uint32_t k = 0; k < n_sel; ++k) {
    st = ilcc_bag_topic_read(iter.it, selected[k], nullptr, 0, &raw[k]);
    if (st != ILCC_OK && st != ILCC_CAPACITY) return st;
  }
  std::vector<uint32_t> batch_first(n_sel + 1);
  uint32_t n_batches = 0;
  st = ilcc_image_sequence_cut(raw.data(), n_sel, per_image, sp.staging_bytes, sp.device_bytes, batch_first.data(), &n_batches);
  if (st == ILCC_CAPACITY)
    return fail(st, "one image (" + std::to_string(per_image) + " device bytes, messages up to " + std::to_string(*std::max_element(raw.begin(), raw.end())) +
                        " bytes) is above staging_bytes or device_bytes");
  if (st != ILCC_OK) return fail(st, "the selection could not be cut into batches");
  uint64_t blob_cap = 256;
  uint32_t images_cap = 1;
  for (uint32_t b = 0; b < n_batches; ++b) {
    uint64_t bytes = 0;
    for (uint32_t k = batch_first[b]; k < batch_first[b + 1]; ++k) bytes += align256(raw[k]);
    blob_cap = std::max(blob_cap, bytes);
    images_cap = std::max(images_cap, batch_first[b + 1] - batch_first[b]);
  }

  std::vector<ilcc_image_record> records(n_sel);
  std::memset(static_cast<void*>(records.data()), 0, sizeof(ilcc_image_record) * n_sel);
  for (ilcc_image_record& r : records) r.distance = -1;

  // one set of allocations for the whole call
  if ((st = select_device(device)) != ILCC_OK) return st;
  hipError_t e;
  Stream stream;
  if ((e = hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking)) != hipSuccess) return hip_fail(e);
  BatchBuffers B[2];
  Worker worker;   // after B: it is joined before the buffers it reads go away
  StructureRoute structure;   // reserved0 == 1: K18 recovers the boards instead of the host thread
  const int n_sets = n_batches > 1 ? 2 : 1;
  for (int k = 0; k < n_sets; ++k) {
    BatchBuffers& b = B[k];
    if ((e = hipHostMalloc((void**)&b.h_blob, blob_cap, hipHostMallocDefault)) != hipSuccess || (e = hipMalloc(&b.d_blob.p, blob_cap)) != hipSuccess ||
        (e = hipMalloc(&b.d_mono.p, mono_pitch * images_cap)) != hipSuccess)
      return hip_fail(e);
    if (!(b.plan = ilcc_image_corner_plan_create(images_cap, w, h))) return ILCC_HIP_ERROR;
    b.capacity = kFirstCapacity;
    b.corners.resize((size_t)images_cap * b.capacity);
    b.n_corners.resize(images_cap);
  }

  for (uint32_t bi = 0; bi < n_batches; ++bi) {
    BatchBuffers& now = B[bi % n_sets];
    now.first = batch_first[bi];
    now.count = batch_first[bi + 1] - batch_first[bi];
    // stage: data[] of every image at 256-byte aligned offsets of one blob
    std::vector<uint64_t> at(now.count);
    std::vector<ilcc_image_layout> lay(now.count);
    uint64_t bytes = 0;
    for (uint32_t m = 0; m < now.count; ++m) {
      const uint32_t k = now.first + m;
      ilcc_image_layout& L = lay[m];
      if ((st = read(k, &L)) != ILCC_OK) return st;
      if (L.width != first.width || L.height != first.height)
        return fail(ILCC_BAD_ARGUMENT, message_name(selected[k]) + ": image " + std::to_string(L.width) + " x " + std::to_string(L.height) + " differs from the first selected image's " +
                                           std::to_string(w) + " x " + std::to_string(h));
      if (L.encoding != first.encoding)
        return fail(ILCC_BAD_ARGUMENT, message_name(selected[k]) + ": its encoding differs from the first selected image's");
      if (L.step > (uint32_t)INT32_MAX || bytes + L.data_bytes > blob_cap) return fail(ILCC_BAD_ARGUMENT, message_name(selected[k]) + ": image data[] larger than its message");
      at[m] = bytes;
      std::memcpy(now.h_blob + bytes, msg.data() + L.data_offset, L.data_bytes);
      bytes = align256(bytes + L.data_bytes);
      ilcc_image_record& r = records[k];
      r.message = (uint32_t)selected[k];
      r.stamp_sec = L.stamp_sec;
      r.stamp_nsec = L.stamp_nsec;
      (void)ilcc_bag_topic_time(iter.it, selected[k], &r.time_sec, &r.time_nsec);
    }
    // one copy, K11 per image, K10b: all on the call's stream
    const uint64_t used = std::min(bytes, blob_cap);
    if ((e = hipMemcpyAsync(now.d_blob.p, now.h_blob, used, hipMemcpyHostToDevice, stream.s)) != hipSuccess) return hip_fail(e);
    for (uint32_t m = 0; m < now.count; ++m) {
      st = ilcc_image_to_mono8_device((const uint8_t*)now.d_blob.p + at[m], w, h, (int32_t)lay[m].step, (int32_t)lay[m].encoding, camera,
                                      (uint8_t*)now.d_mono.p + mono_pitch * m, w, stream.s);
      if (st != ILCC_OK) return fail(st, message_name(selected[now.first + m]) + ": " + ilcc_last_error(nullptr));
    }
    st = ilcc_image_corners_batch_device(now.d_mono.p, mono_pitch, now.count, w, h, w, now.corners.data(), now.capacity, now.n_corners.data(), now.plan,
                                         stream.s);
    if (st == ILCC_CAPACITY) {   // a fuller image than expected: room for the fullest, and the batch once more
      now.capacity = *std::max_element(now.n_corners.begin(), now.n_corners.begin() + now.count);
      now.corners.resize((size_t)images_cap * now.capacity);
      st = ilcc_image_corners_batch_device(now.d_mono.p, mono_pitch, now.count, w, h, w, now.corners.data(), now.capacity, now.n_corners.data(), now.plan,
                                           stream.s);
    }
    if (st != ILCC_OK) return st;
    ++out->n_batches;
    if (sp.reserved0 == 1) {   // structure recovery of this batch on the device (K18), on the call's stream
      if ((st = structure.recover(now.corners.data(), now.capacity, now.n_corners.data(), now.count, images_cap, board_w, board_h,
                                  records.data() + now.first, stream.s)) != ILCC_OK)
        return st;
      continue;
    }
    // structure recovery of this batch on a host thread, while the next batch is staged and runs
    worker.join();
    if (worker.status != ILCC_OK) return fail(worker.status, worker.error);
    worker.t = std::thread(recover, &now, board_w, board_h, records.data(), &worker);
  }
  worker.join();
  if (worker.status != ILCC_OK) return fail(worker.status, worker.error);
  out->host_recovery_ms = worker.ms + structure.ms;

  // fusion of the boards that were found
  const uint32_t N2 = (uint32_t)(2 * board_w * board_h);
  std::vector<double> xy((size_t)n_sel * N2);
  std::vector<int32_t> rows(n_sel), cols(n_sel);
  std::vector<uint8_t> accepted(n_sel), used(n_sel);
  std::vector<double> dist(n_sel);
  for (uint32_t k = 0; k < n_sel; ++k) {
    accepted[k] = records[k].status == ILCC_OK ? 1 : 0;
    rows[k] = records[k].rows;
    cols[k] = records[k].cols;
    std::memcpy(&xy[(size_t)k * N2], records[k].xy, sizeof(double) * N2);
  }
  ilcc_fused_image_corners fused;
  st = ilcc_fuse_image_corners(xy.data(), rows.data(), cols.data(), accepted.data(), n_sel, (uint32_t)board_w, (uint32_t)board_h, sp.gate_px > 0 ? sp.gate_px : 0.0,
                               &fused, used.data(), dist.data());
  out->n_ok = fused.n_ok;
  out->n_used = fused.n_used;
  out->ref_image = fused.ref_image;
  out->rows = fused.rows;
  out->cols = fused.cols;
  out->gate = fused.gate;
  out->spread_rms = fused.spread_rms;
  out->spread_max = fused.spread_max;
  std::memcpy(out->xy, fused.xy, sizeof(fused.xy));
  if (per_image_out)
    for (uint32_t k = 0; k < n_sel; ++k) {
      records[k].accepted = accepted[k];
      records[k].used = used[k];
      records[k].distance = dist[k];
      per_image_out[k] = records[k];
    }
  if (st == ILCC_AMBIGUOUS) return fail(st, "the images' boards do not agree on one corner set (the board or the camera moved, or no majority within the gate)");
  if (st == ILCC_BOARD_NOT_FOUND) return fail(st, "no image holds the board");
  if (st != ILCC_OK) return fail(st, "fusion refused its input");
  return ILCC_OK;
}

}  // namespace

extern "C" {

void ilcc_default_image_sequence_params(ilcc_image_sequence_params* sp) {
  if (!sp) return;
  std::memset(sp, 0, sizeof(*sp));
  sp->stride = 1;
  sp->staging_bytes = kDefaultStagingBytes;
  sp->device_bytes = kDefaultDeviceBytes;
}

int32_t ilcc_bag_corners_all_images(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera, int32_t board_w,
                                    int32_t board_h, const ilcc_image_sequence_params* sp, ilcc_image_sequence_result* out,
                                    ilcc_image_record* per_image_out, uint32_t cap) {
  if (!out) return fail(ILCC_BAD_ARGUMENT, "null argument");
  std::memset(out, 0, sizeof(*out));
  out->ref_image = -1;
  int32_t st;
  if (!bag_path || !topic || !sp || (per_image_out == nullptr && cap != 0)) {
    st = fail(ILCC_BAD_ARGUMENT, "null argument");
  } else if (board_w < 3 || board_h < 3 || (int64_t)board_w * board_h > ILCC_MAX_CORNERS) {
    st = fail(ILCC_BAD_ARGUMENT, "the board must have 3 x 3 .. ILCC_MAX_CORNERS corners");
  } else if (!std::isfinite(sp->gate_px)) {
    st = fail(ILCC_BAD_ARGUMENT, "gate_px is not finite");
  } else if (sp->reserved0 > 1) {
    st = fail(ILCC_BAD_ARGUMENT, "reserved0 (the route of structure recovery) must be 0, the host thread, or 1, K18");
  } else {
    try {   // no exception crosses the C-ABI
      st = all_images(device, bag_path, topic, camera, board_w, board_h, *sp, out, per_image_out, cap);
    } catch (const std::bad_alloc&) {
      st = fail(ILCC_IO_ERROR, "out of memory");
    } catch (...) {
      st = fail(ILCC_IO_ERROR, "image sequence: unknown failure");
    }
  }
  out->status = st;
  return st;
}

}  // extern "C"
