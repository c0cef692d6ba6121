// jpeg_sequence_api.cpp -- ilcc_bag_corners_all_compressed_images (include/ilcc_jpeg_sequence.h): every CompressedImage of a bag
// topic through the decode pool, K13b, K11 and K10b, structure recovery per image, then ilcc_fuse_image_corners.  The layers
// below do the work: the topic iterator (bag_reader.cpp), the message and JPEG header parsers (jpeg_host.cpp, jpeg_entropy.cpp),
// ilcc_jpeg_entropy_decode_many (jpeg_decode_pool.cpp), K13b (k13b_jpeg_batch.hip), K11 (k11_camera_image.hip), K10b
// (k10b_image_corners_batch.hip), ilcc_chessboard_from_corners (image_corners_host.cpp), the cut and the fusion
// (image_sequence_host.cpp).  This file owns the batching, as image_sequence_api.cpp does for raw images: the two sets of
// buffers, and the order of the calls that lets the pool decode batch k + 1 and a host thread recover batch k - 1's boards
// while the device works on batch k.  The guards, the selection and "message i in a vector" are host_util.h's.  Failures below
// are reported through ilcc_last_error(NULL).
// With sp->reserved0 == 1 the Huffman decode is K16's (k16_jpeg_huffman.hip): the pool's threads only run ilcc_jpeg_scan_prepare
// (jpeg_scan_prepare.cpp) into the blob, which then holds files' scans instead of coefficients.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "host_util.h"
#include "ilcc_jpeg_huffman.h"
#include "ilcc_jpeg_sequence.h"
#include "ilcc_sequence.h"
#include "jpeg_entropy.h"
#include "structure_route.h"

using namespace ilcc;

namespace {

constexpr int32_t kFirstCapacity = 1024;   // corners per image; a batch with a fuller image runs again with room for it
constexpr uint64_t kQuantBytes = 3 * 64 * sizeof(uint16_t);   // an image's table rows

// what one image takes, in bytes; every part a multiple of 256
struct Sizes {
  uint64_t coef, staged, planes, pixels, mono, corners, device;
};

bool sizes_of(const ilcc_jpeg_info& I, Sizes* S) {
  if (!jpeg_laid_out(I)) return false;
  const uint64_t bpp = I.n_components == 1 ? 1 : 3, area = (uint64_t)I.width * (uint64_t)I.height;
  S->coef = align256(I.coef_count * sizeof(int16_t));
  S->staged = S->coef + align256(kQuantBytes);
  S->planes = ilcc_jpeg_scratch_bytes(&I);
  S->pixels = align256(bpp * area);
  S->mono = align256(area);
  S->corners = ilcc_image_corner_scratch_bytes(I.width, I.height);
  S->device = S->staged + S->planes + S->pixels + S->mono + S->corners;
  return true;
}

// Route 1 (K16): what one image stages beside its scan, each part a multiple of 256, and what it takes on the device beside
// what it stages and what route 0 takes: its coefficients' slot is in S.coef, its status and K16's counters are here
constexpr uint64_t kTablesBytes = sizeof(ilcc_jpeg_huffman_tables), kImageRowBytes = sizeof(ilcc_jpeg_huffman_image);
constexpr uint64_t kSegmentBytes = sizeof(ilcc_jpeg_huffman_segment), kK16PerImage = 512;

uint64_t huffman_staged(uint64_t data_bytes, uint32_t n_segments) {
  return align256(data_bytes) + align256(kTablesBytes) + align256(kQuantBytes) + align256(kImageRowBytes) + align256(kSegmentBytes * n_segments);
}

// one of the two sets of buffers
struct BatchBuffers {
  uint8_t* h_blob = nullptr;   // page-locked: [count][coef] then [count][3][64] table rows; route 1: see `Sections`
  DeviceBuffer d_all;          // [ blob | planes | pixels | mono8 ]
  uint8_t *d_blob = nullptr, *d_planes = nullptr, *d_pixels = nullptr, *d_mono = nullptr;
  ilcc_image_corner_plan* plan = nullptr;
  std::vector<ilcc_image_corner> corners;
  std::vector<int32_t> n_corners;
  int32_t capacity = 0;
  uint32_t first = 0, count = 0;   // the batch the device and the recovery thread work on, among the selected images
  // the batch the pool decodes into h_blob: the messages stay while their scans are read
  uint32_t staged_first = 0, staged_count = 0;
  std::vector<std::vector<uint8_t>> msg;
  std::vector<ilcc_jpeg_info> info;
  std::vector<const uint8_t*> jpg;
  std::vector<uint64_t> jpg_bytes, coef_cap;
  std::vector<int16_t*> coef;
  std::vector<int32_t> status;
  // route 1: where the staged batch's parts lie in the blob (host and device alike), and each image's share of them
  struct Sections {
    uint64_t tables = 0, quant = 0, images = 0, segments = 0, scans = 0, used = 0;
    uint32_t n_segments = 0, max_segments = 0;
  } at;
  std::vector<uint64_t> scan_at, scan_cap, scan_bytes;
  std::vector<uint32_t> seg_first, seg_cap, seg_count;
  std::vector<std::string> job_error;
  uint8_t *d_coef = nullptr, *d_k16 = nullptr;   // route 1: the coefficients K16 writes; [status | counters]
  uint32_t* h_status = nullptr;                  // page-locked, behind the blob
  ~BatchBuffers() {
    ilcc_image_corner_plan_destroy(plan);
    if (h_blob) (void)hipHostFree(h_blob);
  }
};

// a host thread beside the calling one; joined whatever makes the call end
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

// the staged batch of B through the pool, on a thread of its own so that the calling thread can drive the device meanwhile
void decode(BatchBuffers* B, uint32_t threads, Worker* w) {
  const auto t0 = std::chrono::steady_clock::now();
  w->status = ilcc_jpeg_entropy_decode_many(B->jpg.data(), B->jpg_bytes.data(), B->info.data(), B->coef.data(), B->coef_cap.data(), B->staged_count,
                                            threads, B->status.data());
  if (w->status != ILCC_OK) w->error = ilcc_last_error(nullptr);   // this thread's text: the lowest failing job's
  w->ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Route 1: ilcc_jpeg_scan_prepare of the staged batch on up to `threads` threads (0: 8; at most 16), each image into its share of
// the blob; a refused image is decoded once by the host decoder, whose status and text are the ones reported (route 0's).  Then the
// image rows, on the calling thread of this function.
void prepare(BatchBuffers* B, uint32_t threads, uint64_t coef_count, Worker* w) {
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t n = B->staged_count;
  threads = std::min<uint32_t>(std::min<uint32_t>(threads ? threads : 8u, 16u), std::max<uint32_t>(n, 1u));
  std::atomic<uint32_t> next{0};
  auto* tables = reinterpret_cast<ilcc_jpeg_huffman_tables*>(B->h_blob + B->at.tables);
  auto* rows = reinterpret_cast<ilcc_jpeg_huffman_segment*>(B->h_blob + B->at.segments);
  auto work = [&]() {
    for (uint32_t m = next.fetch_add(1); m < n; m = next.fetch_add(1)) {
      B->status[m] = ilcc_jpeg_scan_prepare(B->jpg[m], B->jpg_bytes[m], &B->info[m], B->h_blob + B->at.scans + B->scan_at[m], B->scan_cap[m],
                                            &B->scan_bytes[m], rows + B->seg_first[m], B->seg_cap[m], &B->seg_count[m], tables + m);
      if (B->status[m] == ILCC_OK) continue;
      B->job_error[m] = jpeg_last_error();
      try {   // what the host decoder says of the same bytes
        std::vector<int16_t> coef(coef_count);
        const int32_t host = ilcc_jpeg_entropy_decode(B->jpg[m], B->jpg_bytes[m], &B->info[m], coef.data(), coef.size());
        if (host != ILCC_OK) {
          B->status[m] = host;
          B->job_error[m] = jpeg_last_error();
        }
      } catch (...) {
      }
    }
  };
  try {
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (std::thread& t : pool) t.join();
  } catch (...) {
    w->status = ILCC_IO_ERROR;
    w->error = "could not start the threads that prepare the scans";
    return;
  }
  auto* images = reinterpret_cast<ilcc_jpeg_huffman_image*>(B->h_blob + B->at.images);
  B->at.max_segments = 0;
  for (uint32_t m = 0; m < n; ++m) {
    if (B->status[m] != ILCC_OK) {
      // route 0 names the LOWEST failing message: an image below m whose scan is corrupt inside its bits (K16's part, which has not
      // run) comes first, so the images below m are decoded by the host decoder, lowest first
      try {
        std::vector<int16_t> coef(coef_count);
        for (uint32_t i = 0; i < m; ++i) {
          const int32_t host = ilcc_jpeg_entropy_decode(B->jpg[i], B->jpg_bytes[i], &B->info[i], coef.data(), coef.size());
          if (host == ILCC_OK) continue;
          B->status[i] = host;
          B->job_error[i] = jpeg_last_error();
          m = i;
          break;
        }
      } catch (...) {
      }
      w->status = B->status[m];
      w->error = B->job_error[m];
      break;
    }
    images[m] = ilcc_jpeg_huffman_image{B->scan_at[m], (uint32_t)B->scan_bytes[m], B->seg_first[m], B->seg_count[m], 0};
    B->at.max_segments = std::max(B->at.max_segments, B->seg_count[m]);
  }
  w->ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int32_t all_images(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera, int32_t board_w, int32_t board_h,
                   const ilcc_jpeg_sequence_params& jp, ilcc_image_sequence_result* out, ilcc_image_record* per_image_out, uint32_t cap) {
  const ilcc_image_sequence_params& sp = jp.seq;
  const bool k16 = jp.reserved0 == 1;
  Iterator iter;
  int32_t st = ilcc_bag_topic_open(bag_path, topic, kCompressedImageMd5, &iter.it);
  if (st == ILCC_BAD_ARGUMENT) {   // no CompressedImage there: point to the sibling when the topic carries raw images
    Iterator raw;
    if (ilcc_bag_topic_open(bag_path, topic, kImageMd5, &raw.it) == ILCC_OK)
      return fail(ILCC_BAD_ARGUMENT, std::string("topic ") + topic +
                                         " carries sensor_msgs/Image, no sensor_msgs/CompressedImage: ilcc_bag_corners_all_images takes it");
    return ilcc_bag_topic_open(bag_path, topic, kCompressedImageMd5, &raw.it);   // the first refusal, with its text
  }
  if (st != ILCC_OK) return st;
  std::vector<uint64_t> selected;
  if ((st = select_messages(iter.it, sp.first, sp.stride, sp.max_images, "max_images", &selected)) != ILCC_OK) return st;
  const uint32_t n_sel = (uint32_t)selected.size();
  out->n_images = (int32_t)n_sel;
  if (cap < n_sel && (per_image_out || cap)) return fail(ILCC_CAPACITY, "per_image_out holds fewer records than images were selected");

  // message k of the selection and its two headers
  auto read = [&](uint32_t k, std::vector<uint8_t>* msg, ilcc_compressed_image_layout* L, ilcc_jpeg_info* I) -> int32_t {
    uint64_t bytes = 0;
    int32_t s = read_message(iter.it, selected[k], msg, &bytes);
    if (s != ILCC_OK) return s;
    if ((s = ilcc_compressed_image_parse(msg->data(), bytes, L)) != ILCC_OK) return fail(s, message_name(selected[k]) + ": " + ilcc_last_error(nullptr));
    if ((s = ilcc_jpeg_parse(msg->data() + L->data_offset, L->data_bytes, I)) != ILCC_OK)
      return fail(s, message_name(selected[k]) + ": " + ilcc_last_error(nullptr));
    return ILCC_OK;
  };

  // message k of the selection, whose size is known to be at least `expect` bytes, without parsing anything
  auto read_bytes = [&](uint32_t k, std::vector<uint8_t>* msg, uint64_t expect) -> int32_t {
    uint64_t bytes = 0;
    const int32_t s = read_message(iter.it, selected[k], msg, &bytes);
    if (s != ILCC_OK) return s;
    return bytes < expect ? fail(ILCC_IO_ERROR, message_name(selected[k]) + ": the message changed while the bag was read") : ILCC_OK;
  };

  // the first selected image decides size, component count and sampling
  ilcc_jpeg_info first;
  {
    std::vector<uint8_t> msg;
    ilcc_compressed_image_layout L;
    if ((st = read(0, &msg, &L, &first)) != ILCC_OK) return st;
  }
  const int32_t w = first.width, h = first.height, bpp = first.n_components == 1 ? 1 : 3;
  const int32_t encoding = bpp == 1 ? ILCC_ENCODING_MONO8 : ILCC_ENCODING_BGR8;
  if (camera && (camera->width != w || camera->height != h))
    return fail(ILCC_BAD_ARGUMENT, message_name(selected[0]) + ": the camera's width / height differ from the image's");
  Sizes S;
  if (!sizes_of(first, &S)) return fail(ILCC_BAD_ARGUMENT, message_name(selected[0]) + ": the JPEG's layout is not ilcc_jpeg_layout's");
  if (!S.corners)
    return fail(ILCC_BAD_ARGUMENT, message_name(selected[0]) + ": image " + std::to_string(w) + " x " + std::to_string(h) + " is smaller than 34 px a side");

  // the batches, cut before anything is allocated: every image stages the same number of bytes
  // (route 1: every image stages its own file; a message that will be refused when its batch is staged counts as its bytes)
  std::vector<uint64_t> raw(n_sel, S.staged);
  std::vector<uint32_t> segments_of(n_sel, 1);
  std::vector<ilcc_compressed_image_layout> layout_of;   // route 1: the two headers of every message that parsed, kept for stage()
  std::vector<ilcc_jpeg_info> info_of;
  std::vector<uint8_t> parsed;
  uint64_t device_per_image = S.device, largest_staged = S.staged;
  if (k16) {
    largest_staged = 0;
    layout_of.resize(n_sel);
    info_of.resize(n_sel);
    parsed.assign(n_sel, 0);
    std::vector<uint8_t> msg;
    for (uint32_t k = 0; k < n_sel; ++k) {
      ilcc_compressed_image_layout& L = layout_of[k];
      ilcc_jpeg_info& I = info_of[k];
      uint64_t data_bytes = 0, scan_bytes = 0;
      if (read(k, &msg, &L, &I) == ILCC_OK && ilcc_jpeg_scan_bound(&I, L.data_bytes, &scan_bytes, &segments_of[k]) == ILCC_OK) {
        data_bytes = L.data_bytes;
        parsed[k] = 1;
      } else {
        (void)ilcc_bag_topic_read(iter.it, selected[k], nullptr, 0, &data_bytes);
        segments_of[k] = 1;
      }
      raw[k] = huffman_staged(data_bytes, segments_of[k]);
      largest_staged = std::max(largest_staged, raw[k]);
    }
    device_per_image = largest_staged + S.coef + kK16PerImage + S.planes + S.pixels + S.mono + S.corners;
  }
  std::vector<uint32_t> batch_first(n_sel + 1);
  uint32_t n_batches = 0;
  st = ilcc_image_sequence_cut(raw.data(), n_sel, device_per_image, sp.staging_bytes, sp.device_bytes, batch_first.data(), &n_batches);
  if (st == ILCC_CAPACITY)
    return fail(st, "one image (" + std::to_string(device_per_image) + " device bytes, " + std::to_string(largest_staged) + " staged bytes) is above staging_bytes or device_bytes");
  if (st != ILCC_OK) return fail(st, "the selection could not be cut into batches");
  uint32_t images_cap = 1;
  uint64_t blob_cap = 0;   // of a set's blob: the largest batch's staged bytes
  for (uint32_t b = 0; b < n_batches; ++b) {
    images_cap = std::max(images_cap, batch_first[b + 1] - batch_first[b]);
    uint64_t sum = 0;
    for (uint32_t k = batch_first[b]; k < batch_first[b + 1]; ++k) sum += raw[k];
    blob_cap = std::max(blob_cap, sum);
  }
  const uint32_t threads = jp.decode_threads;

  std::vector<ilcc_image_record> records(n_sel);
  std::memset(static_cast<void*>(records.data()), 0, sizeof(ilcc_image_record) * n_sel);
  for (ilcc_image_record& r : records) r.distance = -1;

  // one set of allocations for the whole call
  if ((st = select_device(device)) != ILCC_OK) return st;
  hipError_t e;
  Stream stream;
  if ((e = hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking)) != hipSuccess) return hip_fail(e);
  BatchBuffers B[2];
  Worker decoder, worker;   // after B: they are joined before the buffers they use go away
  StructureRoute structure;   // seq.reserved0 == 1: K18 recovers the boards instead of the host thread
  const int n_sets = n_batches > 1 ? 2 : 1;
  // route 1: [ blob | coefficients | K16's statuses and counters | planes | pixels | mono8 ]
  const uint64_t coef_at = k16 ? blob_cap : 0, k16_at = coef_at + (k16 ? S.coef * images_cap : 0);
  const uint64_t planes_at = k16 ? k16_at + kK16PerImage * images_cap : S.staged * images_cap;
  const uint64_t pixels_at = planes_at + S.planes * images_cap, mono_at = pixels_at + S.pixels * images_cap;
  for (int k = 0; k < n_sets; ++k) {
    BatchBuffers& b = B[k];
    if ((e = hipHostMalloc((void**)&b.h_blob, k16 ? blob_cap + align256(sizeof(uint32_t) * images_cap) : S.staged * images_cap, hipHostMallocDefault)) !=
            hipSuccess ||
        (e = hipMalloc(&b.d_all.p, mono_at + S.mono * images_cap)) != hipSuccess)
      return hip_fail(e);
    b.d_blob = (uint8_t*)b.d_all.p;
    if (k16) {
      b.d_coef = b.d_blob + coef_at;
      b.d_k16 = b.d_blob + k16_at;
      b.h_status = reinterpret_cast<uint32_t*>(b.h_blob + blob_cap);
      b.scan_at.resize(images_cap);
      b.scan_cap.resize(images_cap);
      b.scan_bytes.resize(images_cap);
      b.seg_first.resize(images_cap);
      b.seg_cap.resize(images_cap);
      b.seg_count.resize(images_cap);
      b.job_error.resize(images_cap);
    }
    b.d_planes = b.d_blob + planes_at;
    b.d_pixels = b.d_blob + pixels_at;
    b.d_mono = b.d_blob + mono_at;
    if (!(b.plan = ilcc_image_corner_plan_create(images_cap, w, h))) return ILCC_HIP_ERROR;
    b.capacity = kFirstCapacity;
    b.corners.resize((size_t)images_cap * b.capacity);
    b.n_corners.resize(images_cap);
    b.msg.resize(images_cap);
    b.info.resize(images_cap);
    b.jpg.resize(images_cap);
    b.jpg_bytes.resize(images_cap);
    b.coef.resize(images_cap);
    b.coef_cap.assign(images_cap, first.coef_count);
    b.status.resize(images_cap);
  }

  // reads and checks the messages of batch bi, writes their table rows into the blob and hands their scans to the pool
  auto stage = [&](uint32_t bi) -> int32_t {
    BatchBuffers& b = B[bi % n_sets];
    b.staged_first = batch_first[bi];
    b.staged_count = batch_first[bi + 1] - batch_first[bi];
    if (k16) {   // the blob's parts for this many images: tables, table rows, image rows, segment rows, scans
      const uint64_t n = b.staged_count;
      uint64_t rows = 0;
      for (uint32_t m = 0; m < n; ++m) rows += segments_of[b.staged_first + m];
      b.at.tables = 0;
      b.at.quant = align256(kTablesBytes * n);
      b.at.images = b.at.quant + align256(kQuantBytes * n);
      b.at.segments = b.at.images + align256(kImageRowBytes * n);
      b.at.scans = b.at.segments + align256(kSegmentBytes * rows);
      b.at.n_segments = (uint32_t)rows;
    }
    uint16_t* quant = reinterpret_cast<uint16_t*>(b.h_blob + (k16 ? b.at.quant : S.coef * b.staged_count));
    uint64_t scan_at = 0;
    uint32_t seg_first = 0;
    for (uint32_t m = 0; m < b.staged_count; ++m) {
      const uint32_t k = b.staged_first + m;
      ilcc_compressed_image_layout L;
      ilcc_jpeg_info& I = b.info[m];
      int32_t s = ILCC_OK;
      if (k16 && parsed[k]) {   // the headers are known from the cut: the bytes only
        L = layout_of[k];
        I = info_of[k];
        s = read_bytes(k, &b.msg[m], L.data_offset + L.data_bytes);
      } else {
        s = read(k, &b.msg[m], &L, &I);
      }
      if (s != ILCC_OK) return s;
      if (I.width != w || I.height != h)
        return fail(ILCC_BAD_ARGUMENT, message_name(selected[k]) + ": image " + std::to_string(I.width) + " x " + std::to_string(I.height) +
                                           " differs from the first selected image's " + std::to_string(w) + " x " + std::to_string(h));
      if (I.n_components != first.n_components)
        return fail(ILCC_BAD_ARGUMENT, message_name(selected[k]) + ": " + std::to_string(I.n_components) + " components differ from the first selected image's " +
                                           std::to_string(first.n_components));
      if (I.comp[0].h != first.comp[0].h || I.comp[0].v != first.comp[0].v || I.coef_count != first.coef_count)
        return fail(ILCC_BAD_ARGUMENT, message_name(selected[k]) + ": its chroma sampling differs from the first selected image's");
      b.jpg[m] = b.msg[m].data() + L.data_offset;
      b.jpg_bytes[m] = L.data_bytes;
      if (k16) {
        uint64_t scan_bound = 0;
        uint32_t seg_bound = 0;
        if ((s = ilcc_jpeg_scan_bound(&I, L.data_bytes, &scan_bound, &seg_bound)) != ILCC_OK || seg_bound != segments_of[k])
          return fail(ILCC_IO_ERROR, message_name(selected[k]) + ": the message changed while the bag was read");
        b.scan_at[m] = scan_at;
        b.scan_cap[m] = scan_bound;              // <= data_bytes: inside the image's up(data_bytes) of the blob
        b.seg_first[m] = seg_first;
        b.seg_cap[m] = seg_bound;
        scan_at += align256(L.data_bytes);
        seg_first += seg_bound;
      } else {
        b.coef[m] = reinterpret_cast<int16_t*>(b.h_blob + S.coef * m);
      }
      for (int c = 0; c < 3; ++c)   // a 1-component image: row 0 three times
        std::memcpy(quant + ((size_t)m * 3 + c) * 64, I.quant[I.comp[c < I.n_components ? c : 0].quant_index], 64 * sizeof(uint16_t));
      ilcc_image_record& r = records[k];
      r.message = (uint32_t)selected[k];
      r.stamp_sec = L.stamp_sec;
      r.stamp_nsec = L.stamp_nsec;
      (void)ilcc_bag_topic_time(iter.it, selected[k], &r.time_sec, &r.time_nsec);
    }
    b.at.used = b.at.scans + scan_at;
    decoder.status = ILCC_OK;
    decoder.t = k16 ? std::thread(prepare, &b, threads, (uint64_t)first.coef_count, &decoder) : std::thread(decode, &b, threads, &decoder);
    return ILCC_OK;
  };

  if ((st = stage(0)) != ILCC_OK) return st;
  for (uint32_t bi = 0; bi < n_batches; ++bi) {
    BatchBuffers& now = B[bi % n_sets];
    decoder.join();
    if (decoder.status != ILCC_OK) {
      uint32_t m = 0;
      while (m + 1 < now.staged_count && now.status[m] == ILCC_OK) ++m;
      return fail(decoder.status, message_name(selected[now.staged_first + m]) + ": " + decoder.error);
    }
    // the other set is free for the pool: its batch (bi - 1) has left the device, and recovery reads none of what staging writes
    if (bi + 1 < n_batches && (st = stage(bi + 1)) != ILCC_OK) return st;
    now.first = now.staged_first;
    now.count = now.staged_count;
    // one copy, (route 1: K16,) K13b, K11 per image, K10b: all on the call's stream
    const uint64_t used = k16 ? now.at.used : S.coef * now.count + kQuantBytes * now.count;
    if ((e = hipMemcpyAsync(now.d_blob, now.h_blob, used, hipMemcpyHostToDevice, stream.s)) != hipSuccess) return hip_fail(e);
    if (k16) {
      ilcc_jpeg_huffman_job job{};
      job.layout = &first;
      job.d_scans = now.d_blob + now.at.scans;
      job.scans_bytes = now.at.used - now.at.scans;
      job.d_tables = reinterpret_cast<const ilcc_jpeg_huffman_tables*>(now.d_blob + now.at.tables);
      job.d_segments = reinterpret_cast<const ilcc_jpeg_huffman_segment*>(now.d_blob + now.at.segments);
      job.d_images = reinterpret_cast<const ilcc_jpeg_huffman_image*>(now.d_blob + now.at.images);
      job.d_coef = reinterpret_cast<int16_t*>(now.d_coef);
      job.coef_pitch = S.coef / sizeof(int16_t);
      job.d_status = reinterpret_cast<uint32_t*>(now.d_k16);
      job.d_scratch = now.d_k16 + align256(sizeof(uint32_t) * images_cap);
      job.scratch_bytes = ilcc_jpeg_huffman_scratch_bytes(now.count);
      job.n_images = now.count;
      job.n_segments = now.at.n_segments;
      job.max_segments = now.at.max_segments;
      job.subsequence_bits = 0;
      job.hip_stream = stream.s;
      if ((st = ilcc_jpeg_huffman_batch_device(&job)) != ILCC_OK) return st;
      // the statuses travel back behind K16 and are read once K10b has waited for the stream: nothing waits for K16 alone.  (What
      // K13b, K11 and K10b make of a refused image's unspecified coefficients stays inside its own buffers and is dropped.)
      if ((e = hipMemcpyAsync(now.h_status, now.d_k16, sizeof(uint32_t) * now.count, hipMemcpyDeviceToHost, stream.s)) != hipSuccess) return hip_fail(e);
    }
    // a scan K16 refused ends the call as the host decoder would have: its status, its text, the lowest such message
    auto k16_refusal = [&]() -> int32_t {
      if ((e = hipStreamSynchronize(stream.s)) != hipSuccess) return hip_fail(e);   // K10b has waited already unless it refused on the host
      for (uint32_t m = 0; m < now.count; ++m) {
        if (now.h_status[m] == 0) continue;
        std::vector<int16_t> coef(first.coef_count);
        const int32_t host = ilcc_jpeg_entropy_decode(now.jpg[m], now.jpg_bytes[m], &now.info[m], coef.data(), coef.size());
        if (host != ILCC_OK) return fail(host, message_name(selected[now.first + m]) + ": " + ilcc_last_error(nullptr));
        return fail(ILCC_HIP_ERROR, message_name(selected[now.first + m]) + ": internal error: K16 refused a scan (status " +
                                        std::to_string(now.h_status[m]) + ") that the host decoder accepts");
      }
      return ILCC_OK;
    };
    const uint8_t* d_quant = now.d_blob + (k16 ? now.at.quant : S.coef * now.count);
    st = ilcc_jpeg_idct_batch_device(&first, reinterpret_cast<const uint16_t*>(d_quant), reinterpret_cast<const int16_t*>(k16 ? now.d_coef : now.d_blob),
                                     S.coef / sizeof(int16_t), now.count, now.d_pixels, S.pixels, bpp * w, now.d_planes, S.planes * images_cap, stream.s);
    if (st != ILCC_OK) return st;
    for (uint32_t m = 0; m < now.count; ++m) {
      st = ilcc_image_to_mono8_device(now.d_pixels + S.pixels * m, w, h, bpp * w, encoding, camera, now.d_mono + S.mono * m, w, stream.s);
      if (st != ILCC_OK) return fail(st, message_name(selected[now.first + m]) + ": " + ilcc_last_error(nullptr));
    }
    st = ilcc_image_corners_batch_device(now.d_mono, S.mono, now.count, w, h, w, now.corners.data(), now.capacity, now.n_corners.data(), now.plan, stream.s);
    if (k16) {
      const int32_t refused = k16_refusal();
      if (refused != ILCC_OK) return refused;
    }
    if (st == ILCC_CAPACITY) {   // a fuller image than expected: room for the fullest, and the batch once more
      now.capacity = *std::max_element(now.n_corners.begin(), now.n_corners.begin() + now.count);
      now.corners.resize((size_t)images_cap * now.capacity);
      st = ilcc_image_corners_batch_device(now.d_mono, S.mono, now.count, w, h, w, now.corners.data(), now.capacity, now.n_corners.data(), now.plan, stream.s);
    }
    if (st != ILCC_OK) return st;
    ++out->n_batches;
    if (jp.seq.reserved0 == 1) {   // structure recovery of this batch on the device (K18), on the call's stream
      if ((st = structure.recover(now.corners.data(), now.capacity, now.n_corners.data(), now.count, images_cap, board_w, board_h,
                                  records.data() + now.first, stream.s)) != ILCC_OK)
        return st;
      continue;
    }
    // structure recovery of this batch on a host thread, while the next batch runs
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
  std::vector<uint8_t> accepted(n_sel), used_flags(n_sel);
  std::vector<double> dist(n_sel);
  for (uint32_t k = 0; k < n_sel; ++k) {
    accepted[k] = records[k].status == ILCC_OK ? 1 : 0;
    rows[k] = records[k].rows;
    cols[k] = records[k].cols;
    std::memcpy(&xy[(size_t)k * N2], records[k].xy, sizeof(double) * N2);
  }
  ilcc_fused_image_corners fused;
  st = ilcc_fuse_image_corners(xy.data(), rows.data(), cols.data(), accepted.data(), n_sel, (uint32_t)board_w, (uint32_t)board_h, sp.gate_px > 0 ? sp.gate_px : 0.0,
                               &fused, used_flags.data(), dist.data());
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
      records[k].used = used_flags[k];
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

void ilcc_default_jpeg_sequence_params(ilcc_jpeg_sequence_params* jp) {
  if (!jp) return;
  std::memset(jp, 0, sizeof(*jp));
  ilcc_default_image_sequence_params(&jp->seq);
}

int32_t ilcc_jpeg_sequence_bytes(const ilcc_jpeg_info* layout, uint64_t* staged_bytes, uint64_t* device_bytes) {
  Sizes S;
  if (!layout || !staged_bytes || !device_bytes) return fail(ILCC_BAD_ARGUMENT, "ilcc_jpeg_sequence_bytes: null argument");
  if (!sizes_of(*layout, &S)) return fail(ILCC_BAD_ARGUMENT, "ilcc_jpeg_sequence_bytes: the layout's block counts and offsets are not ilcc_jpeg_layout's");
  *staged_bytes = S.staged;
  *device_bytes = S.device;
  return ILCC_OK;
}

int32_t ilcc_jpeg_huffman_sequence_bytes(const ilcc_jpeg_info* layout, uint64_t data_bytes, uint32_t n_segments, uint64_t* staged_bytes,
                                         uint64_t* device_bytes) {
  Sizes S;
  if (!layout || !staged_bytes || !device_bytes) return fail(ILCC_BAD_ARGUMENT, "ilcc_jpeg_huffman_sequence_bytes: null argument");
  if (!sizes_of(*layout, &S))
    return fail(ILCC_BAD_ARGUMENT, "ilcc_jpeg_huffman_sequence_bytes: the layout's block counts and offsets are not ilcc_jpeg_layout's");
  *staged_bytes = huffman_staged(data_bytes, n_segments);
  *device_bytes = *staged_bytes + S.coef + kK16PerImage + S.planes + S.pixels + S.mono + S.corners;
  return ILCC_OK;
}

int32_t ilcc_bag_corners_all_compressed_images(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera, int32_t board_w,
                                               int32_t board_h, const ilcc_jpeg_sequence_params* sp, ilcc_image_sequence_result* out,
                                               ilcc_image_record* per_image_out, uint32_t cap) {
  if (!out) return fail(ILCC_BAD_ARGUMENT, "null argument");
  std::memset(out, 0, sizeof(*out));
  out->ref_image = -1;
  int32_t st;
  if (!bag_path || !topic || !sp || (per_image_out == nullptr && cap != 0)) {
    st = fail(ILCC_BAD_ARGUMENT, "null argument");
  } else if (board_w < 3 || board_h < 3 || (int64_t)board_w * board_h > ILCC_MAX_CORNERS) {
    st = fail(ILCC_BAD_ARGUMENT, "the board must have 3 x 3 .. ILCC_MAX_CORNERS corners");
  } else if (!std::isfinite(sp->seq.gate_px)) {
    st = fail(ILCC_BAD_ARGUMENT, "gate_px is not finite");
  } else if (sp->reserved0 > 1) {
    st = fail(ILCC_BAD_ARGUMENT, "reserved0 (the route of the Huffman decode) must be 0, the host pool, or 1, K16");
  } else if (sp->seq.reserved0 > 1) {
    st = fail(ILCC_BAD_ARGUMENT, "seq.reserved0 (the route of structure recovery) must be 0, the host thread, or 1, K18");
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
