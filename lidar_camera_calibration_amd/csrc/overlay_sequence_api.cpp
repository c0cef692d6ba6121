// overlay_sequence_api.cpp -- ilcc_bag_pcd2image_all_pairs (include/ilcc_overlay_sequence.h): every selected scan of a recording
// drawn on the image whose header stamp is nearest to its own, and written as a JPEG file's bytes.  The recording, its batches (cut
// BEFORE anything is allocated, here with a device budget and K17's 65535 images), the staging and the upload with K0b and K11c
// are the paired front end's (paired_front.h); an unpaired scan is never staged: it costs a record.  The rows and scans of a batch
// become the files' bytes in the JPEG finisher (jpeg_finish.h).  This file owns K12b (k12b_overlay_batch.hip), K14b
// (k14b_jpeg_write_batch.hip) and K17 (k17_jpeg_huffman_enc.hip) with their buffers (a paired scan's bytes:
// overlay_sequence_host.cpp), and the order of the calls that lets the host stage the next batch while the device works on this one.
// Failures below are reported through ilcc_last_error(NULL).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ilcc_overlay_sequence.h"
#include "jpeg_finish.h"
#include "paired_front.h"

using namespace ilcc;

namespace {

// what one picture takes on the device, every part a multiple of 256 (overlay_sequence_host.cpp sums the same parts)
struct Sizes {
  uint64_t canvas, owner, coef, fdct, out_per_image;
};

// one of the two sets of buffers
struct Buffers : PairedBuffers {
  Pinned h_back, h_pixels;      // h_back: [ rows | scans ]
  DeviceBuffer d_pictures;      // [ canvases | owner | coefficients | K14b's planes | scans | rows | K17's scratch ]
  uint64_t owner_at = 0, coef_at = 0, fdct_at = 0, out_at = 0, rows_at = 0, k17_at = 0, k17_bytes = 0;
  ilcc_overlay_plan* overlay = nullptr;
  std::vector<uint32_t> n_drawn;
  JpegFinisher files;
  ~Buffers() { ilcc_overlay_plan_destroy(overlay); }
};

int32_t all_pairs(int32_t device, const char* image_bag, const char* image_topic, const char* lidar_bag, const char* lidar_topic,
                  const ilcc_camera_model* camera, const double* T, double distance_valid, int32_t quality, const ilcc_overlay_sequence_params& sp,
                  ilcc_overlay_sink sink, void* user, uint32_t* n_scans, uint32_t* n_paired) {
  PairedRecording c;
  int32_t st = c.open("ilcc_bag_pcd2image_all_pairs", image_bag, image_topic, lidar_bag, lidar_topic, camera, T, sp.first, sp.stride, sp.max_scans, sp.max_dt_ns);
  if (st != ILCC_OK) return st;

  // the file every picture becomes: 3 components, 4:2:0, no restart markers, as ilcc_jpeg_write_file writes it
  const int32_t w = camera->width, h = camera->height;
  ilcc_jpeg_info info;
  if ((st = ilcc_jpeg_write_info(w, h, 3, 2, 2, quality, 0, &info)) != ILCC_OK) return st;
  const uint64_t pixels = (uint64_t)w * (uint64_t)h;
  Sizes S;
  S.canvas = align256(3 * pixels);
  S.owner = align256(4 * pixels);   // a multiple of 16: K12b's plane pitch is ilcc_overlay_batch_scratch_bytes(w, h, 1) <= this
  S.coef = align256(info.coef_count * sizeof(int16_t));
  S.fdct = align256(ilcc_jpeg_fdct_scratch_bytes(&info));
  S.out_per_image = align16(sp.out_bytes_per_image ? sp.out_bytes_per_image : pixels);
  const uint64_t per_scan = ilcc_overlay_sequence_bytes(w, h, sp.out_bytes_per_image);
  if (per_scan == 0) return fail(ILCC_BAD_ARGUMENT, "image too large for K17, or out_bytes_per_image of 2^40 or more");
  *n_scans = (uint32_t)c.selected.size();
  *n_paired = c.n_paired();

  std::vector<PairedBatch> batches;
  PairedLargest largest;
  PairedBudgets budgets;
  budgets.staging = sp.staging_bytes;
  budgets.image = sp.image_bytes;
  budgets.device = sp.device_bytes ? sp.device_bytes : 1ull << 30;
  budgets.per_member = per_scan;
  budgets.member_cap = 65535;
  if ((st = c.cut(budgets, &batches, &largest)) != ILCC_OK) return st;

  // one set of allocations for the whole call
  if ((st = select_device(device)) != ILCC_OK) return st;
  hipError_t e;
  Stream stream;
  if ((e = hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking)) != hipSuccess) return hip_fail(e);
  Buffers B[2];
  const int sets = batches.size() > 1 ? 2 : 1;
  const uint64_t mm = std::max<uint32_t>(largest.members, 1), out_cap_max = S.out_per_image * mm;
  const bool keep_pixels = sp.keep_pixels != 0;
  for (int k = 0; k < sets && largest.members; ++k) {
    Buffers& b = B[k];
    b.owner_at = S.canvas * mm;
    b.coef_at = b.owner_at + S.owner * mm;
    b.fdct_at = b.coef_at + S.coef * mm;
    b.out_at = b.fdct_at + S.fdct * mm;
    b.rows_at = b.out_at + align256(out_cap_max);
    b.k17_at = b.rows_at + align256(sizeof(ilcc_jpeg_encode_row) * mm);
    b.k17_bytes = ilcc_jpeg_huffman_encode_scratch_bytes(&info, (uint32_t)mm, out_cap_max);
    if (b.k17_bytes == 0) return fail(ILCC_BAD_ARGUMENT, "a batch's pictures are too large for K17");
    const uint64_t back_rows = align256(sizeof(ilcc_jpeg_encode_row) * mm);
    if ((st = b.allocate(largest)) != ILCC_OK) return st;
    if ((e = hipHostMalloc((void**)&b.h_back.p, back_rows + out_cap_max, hipHostMallocDefault)) != hipSuccess ||
        (keep_pixels && (e = hipHostMalloc((void**)&b.h_pixels.p, S.canvas * mm, hipHostMallocDefault)) != hipSuccess) ||
        (e = hipMalloc(&b.d_pictures.p, b.k17_at + b.k17_bytes)) != hipSuccess)
      return hip_fail(e);
    if (!(b.overlay = ilcc_overlay_plan_create((uint32_t)mm, std::max<uint64_t>(largest.points, 1)))) return ILCC_HIP_ERROR;
    const uint8_t* base = static_cast<const uint8_t*>(b.d_pictures.p);
    b.files.info = &info;
    b.files.stream = stream.s;
    b.files.d_coef = base + b.coef_at;
    b.files.coef_pitch = S.coef;
    b.files.d_scans = base + b.out_at;
    b.files.d_rows = reinterpret_cast<const ilcc_jpeg_encode_row*>(base + b.rows_at);
    b.files.out_per_image = S.out_per_image;
    b.files.h_back = b.h_back.p;
    b.files.back_rows = back_rows;
    if ((st = b.files.init()) != ILCC_OK) return st;
  }
  InFlight flying;   // declared behind the buffers: its destructor runs before theirs
  flying.s = stream.s;

  // everything the device does for the batch B carries up to the rows, queued on the stream
  const auto submit = [&](Buffers* B) -> int32_t {
    const uint32_t m = (uint32_t)B->batch->members.size();
    if (m == 0) return ILCC_OK;
    PairedImages im;
    int32_t s = c.upload(B, camera, stream.s, &im);
    if (s != ILCC_OK) return s;
    uint8_t* base = static_cast<uint8_t*>(B->d_pictures.p);
    ilcc_overlay_batch_job oj{};
    oj.d_xyzi = B->d_xyzi.p;
    oj.offsets = B->offsets.data();
    oj.d_images_bgr = im.image_ptrs.data();
    oj.image_steps = im.steps.data();
    oj.image_of_scan = im.image_of_scan.data();
    oj.cam = &c.proj;
    oj.d_canvas = base;
    oj.d_scratch = base + B->owner_at;
    oj.plan = B->overlay;
    oj.hip_stream = stream.s;
    oj.canvas_pitch = S.canvas;
    oj.scratch_bytes = S.owner * m;
    oj.distance_valid = distance_valid;
    oj.inten_low = 0.0;    // pcd2image.cpp fixes the colour range
    oj.inten_high = 60.0;
    oj.n_scans = m;
    oj.n_images = (uint32_t)im.image_ptrs.size();
    oj.canvas_stride = 3 * w;
    if ((s = ilcc_overlay_batch_device(&oj)) != ILCC_OK) return s;
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
    fj.hip_stream = stream.s;
    if ((s = ilcc_jpeg_fdct_batch_device(&fj)) != ILCC_OK) return s;
    if (sp.route != 0) return ILCC_OK;
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
    hj.hip_stream = stream.s;
    if ((s = ilcc_jpeg_huffman_encode_batch_device(&hj)) != ILCC_OK) return s;
    return B->files.rows_back(m);
  };

  std::vector<std::vector<uint8_t>> files(mm);   // of the batch being handed to the sink
  std::vector<uint32_t> route_of(mm);

  // the batches: while the device works on batch k the host reads and stages batch k + 1; while it works on k + 1 the host sinks k
  if ((st = c.stage(&B[0], batches[0])) != ILCC_OK || (st = submit(&B[0])) != ILCC_OK) return st;
  for (size_t k = 0; k < batches.size(); ++k) {
    Buffers& now = B[k & 1];
    Buffers& next = B[(k + 1) & 1];   // its previous batch has been finished, copied back and handed to the sink
    const bool more = k + 1 < batches.size();
    const int32_t st_next = more ? c.stage(&next, batches[k + 1]) : ILCC_OK;
    const PairedBatch& b = *now.batch;
    const uint32_t m = (uint32_t)b.members.size();
    if (m) {
      now.n_drawn.assign(m, 0);
      if ((st = ilcc_overlay_plan_finish(now.overlay, now.n_drawn.data())) != ILCC_OK) return st;
      if ((e = hipStreamSynchronize(stream.s)) != hipSuccess) return hip_fail(e);   // only this batch is on the stream: the rows are here
      if (keep_pixels && (e = hipMemcpyAsync(now.h_pixels.p, now.d_pictures.p, S.canvas * m, hipMemcpyDeviceToHost, stream.s)) != hipSuccess) return hip_fail(e);
      bool queued = false;
      if (sp.route == 0 && (st = now.files.scans_back(m, &queued)) != ILCC_OK) return st;
      if ((e = hipStreamSynchronize(stream.s)) != hipSuccess) return hip_fail(e);
      for (uint32_t i = 0; i < m; ++i) {   // the sink is called in scan order below, so every file's bytes are held: the three spans concatenated
        JpegFile f;
        if ((st = now.files.file(i, sp.route, "cloud message " + std::to_string(c.selected[b.members[i]]), &files[i], &f)) != ILCC_OK) return st;
        route_of[i] = f.route;
        if (f.route == 1) continue;   // the host encoder's bytes are in files[i] already
        files[i].resize(f.bytes());
        uint64_t at = 0;
        for (int p = 0; p < 3; ++p) {
          std::memcpy(files[i].data() + at, f.part[p], f.part_bytes[p]);
          at += f.part_bytes[p];
        }
      }
    }
    if (st_next != ILCC_OK) return st_next;
    if (more && (st = submit(&next)) != ILCC_OK) return st;   // the device goes on while the host sinks
    uint32_t member = 0;
    for (uint32_t s = 0; s < b.scans; ++s) {
      const uint32_t g = b.first_scan + s;
      ilcc_overlay_record r;
      c.fill(g, &r);
      const uint8_t* jpeg = nullptr;
      const uint8_t* bgr = nullptr;
      if (c.pair[g] >= 0) {
        r.n_drawn = now.n_drawn[member];
        r.route = route_of[member];
        r.file_bytes = files[member].size();
        jpeg = files[member].data();
        if (keep_pixels) bgr = now.h_pixels.p + S.canvas * member;
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
