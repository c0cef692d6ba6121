// sequence_api.cpp -- ilcc_bag_corners_all_scans (include/ilcc_sequence.h): every scan of a bag topic through the ordinary batch
// pipeline, then ilcc_fuse_corners.  The layers below do the work: the topic iterator (bag_reader.cpp), K0b (k0b_unpack_batch.hip),
// ilcc_submit_batch_device / ilcc_wait (ilcc_api.cpp), the fusion (sequence_host.cpp).  This file owns the batching: which scans
// form a batch, the two sets of staging buffers, and the order of the calls that lets the host read the next batch while the
// device works on this one.  The guards, the selection and "message i in a vector" are host_util.h's.  Failures below are
// reported through ilcc_last_error(NULL).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "host_util.h"
#include "ilcc_seed.h"
#include "ilcc_sequence.h"
#include "k15_seed.h"   // HandleView

using namespace ilcc;

namespace {

constexpr uint64_t kDefaultStagingBytes = 256ull << 20;

// one of the two sets of staging buffers, and the batch it currently carries
struct BatchBuffers {
  uint8_t* h_blob = nullptr;   // page-locked
  DeviceBuffer d_blob, d_xyzi;
  ilcc_unpack_plan* plan = nullptr;
  std::vector<ilcc_pointcloud2_layout> layouts;
  std::vector<uint64_t> src, offsets;
  uint64_t bytes = 0, points = 0;
  uint32_t first_scan = 0;     // of the batch among the selected scans
  ~BatchBuffers() {
    ilcc_unpack_plan_destroy(plan);
    if (h_blob) (void)hipHostFree(h_blob);
  }
  uint32_t scans() const { return (uint32_t)layouts.size(); }
};

// a batch the pipeline still works on must be waited for before its buffers go away, whatever made the call end (host_util.h's
// InFlight waits for a stream; this one for the pipeline's ticket)
struct TicketInFlight {
  ilcc_handle* h;
  int32_t ticket = -1;
  std::vector<ilcc_result> sink;
  ~TicketInFlight() {
    if (ticket >= 0 && !sink.empty()) (void)ilcc_wait(h, ticket, sink.data());
  }
};

struct Chain {
  ilcc_handle* h;
  HandleView hv;
  ilcc_bag_topic* it;
  std::vector<uint64_t> selected;   // message indices
  uint64_t blob_cap = 0, xyzi_cap = 0;
  uint32_t frames_cap = 0;
  // the message read last and not yet staged (it did not fit the batch that was being filled)
  std::vector<uint8_t> msg;
  ilcc_pointcloud2_layout pending;
  bool have_pending = false;
  uint32_t next_scan = 0;
  std::vector<ilcc_scan_record>* records;

  int32_t fetch(uint32_t scan) {   // message of selected scan `scan` -> msg, pending
    uint64_t bytes = 0;
    int32_t st = read_message(it, selected[scan], &msg, &bytes);
    if (st != ILCC_OK) return st;
    if ((st = ilcc_pointcloud2_parse(msg.data(), bytes, &pending)) != ILCC_OK) return st;
    have_pending = true;
    return ILCC_OK;
  }

  // fills B with as many of the next scans as fit
  int32_t stage(BatchBuffers* B) {
    B->layouts.clear();
    B->src.clear();
    B->bytes = B->points = 0;
    B->first_scan = next_scan;
    while (next_scan < selected.size() && B->scans() < frames_cap) {
      int32_t st;
      if (!have_pending && (st = fetch(next_scan)) != ILCC_OK) return st;
      const uint64_t pts = (uint64_t)pending.height * pending.width, at = align16(B->bytes);
      if (pts > hv.max_points) return fail(ILCC_CAPACITY, "a scan holds more points than the handle's max_total_points");
      if (pts > xyzi_cap || pending.data_bytes > blob_cap) return fail(ILCC_CAPACITY, "a scan does not fit the staging buffers (point_step below 4?)");
      if (B->scans() > 0 && (at + pending.data_bytes > blob_cap || B->points + pts > xyzi_cap)) break;
      if (pending.data_bytes) std::memcpy(B->h_blob + at, msg.data() + pending.data_offset, pending.data_bytes);
      B->layouts.push_back(pending);
      B->src.push_back(at);
      B->bytes = at + pending.data_bytes;
      B->points += pts;
      ilcc_scan_record& r = (*records)[next_scan];
      r.message = (uint32_t)selected[next_scan];
      r.stamp_sec = pending.stamp_sec;
      r.stamp_nsec = pending.stamp_nsec;
      (void)ilcc_bag_topic_time(it, selected[next_scan], &r.time_sec, &r.time_nsec);
      have_pending = false;
      ++next_scan;
    }
    return ILCC_OK;
  }

  // one copy, K0b; complete on return (the pipeline's streams are the handle's own: its inputs must be resident when it is handed them)
  int32_t upload(BatchBuffers* B, hipStream_t s) {
    hipError_t e;
    if (B->bytes && (e = hipMemcpyAsync(B->d_blob.p, B->h_blob, B->bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e);
    B->offsets.assign(B->scans() + 1, 0);
    const int32_t st = ilcc_pointcloud2_unpack_batch_device(B->d_blob.p, B->bytes, B->layouts.data(), B->src.data(), B->scans(), B->d_xyzi.p, xyzi_cap,
                                                            B->offsets.data(), B->plan, s);
    if (st != ILCC_OK) return st;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e);
    return ILCC_OK;
  }
};

bool scan_accepted(const ilcc_result& r, const ilcc_sequence_params& sp, int32_t n_corners) {
  const bool status_ok = r.status == ILCC_OK || (sp.accept_ambiguous && r.status == ILCC_AMBIGUOUS);
  const bool coverage_ok = sp.accept_low_coverage || !(r.flags & ILCC_FLAG_LOW_COVERAGE);
  return status_ok && coverage_ok && r.n_corners == n_corners;
}

int32_t all_scans(ilcc_handle* h, const char* bag_path, const char* topic, const float* click, int32_t seed_mode, const ilcc_sequence_params& sp,
                  ilcc_sequence_result* out, ilcc_scan_record* per_scan_out, uint32_t cap) {
  Iterator iter;
  int32_t st = ilcc_bag_topic_open(bag_path, topic, nullptr, &iter.it);
  if (st != ILCC_OK) return st;
  Chain c;
  c.h = h;
  c.hv = handle_view(h);
  c.it = iter.it;
  if ((st = select_messages(iter.it, sp.first, sp.stride, sp.max_scans, "max_scans", &c.selected)) != ILCC_OK) return st;
  const uint32_t n_sel = (uint32_t)c.selected.size();
  out->n_scans = (int32_t)n_sel;
  if (per_scan_out && cap < n_sel) return fail(ILCC_CAPACITY, "per_scan_out holds fewer records than scans were selected");
  const int32_t n_corners = (c.hv.p.board_w - 1) * (c.hv.p.board_h - 1);
  if (n_corners < 1 || n_corners > ILCC_MAX_CORNERS) return fail(ILCC_BAD_ARGUMENT, "the handle's board has no corner lattice");

  // sizes: the messages' lengths are known from open; their point counts only once they are read
  uint64_t total_bytes = 0, largest = 0;
  for (uint64_t i : c.selected) {
    uint64_t bytes = 0;
    st = ilcc_bag_topic_read(iter.it, i, nullptr, 0, &bytes);
    if (st != ILCC_OK && st != ILCC_CAPACITY) return st;
    total_bytes += align16(bytes);
    largest = std::max(largest, align16(bytes));
  }
  const uint64_t budget = sp.staging_bytes ? sp.staging_bytes : kDefaultStagingBytes;
  c.blob_cap = std::max<uint64_t>(std::max(std::min(budget, total_bytes), largest), 16);
  c.xyzi_cap = std::max<uint64_t>(std::min<uint64_t>(c.hv.max_points, c.blob_cap / 4), 1);   // a point with a float32 field takes >= 4 bytes
  c.frames_cap = std::min<uint32_t>(c.hv.max_frames, n_sel);
  std::vector<ilcc_scan_record> records(n_sel);
  std::memset(static_cast<void*>(records.data()), 0, sizeof(ilcc_scan_record) * n_sel);
  c.records = &records;

  // one set of allocations for the whole call
  hipError_t e;
  if ((e = hipSetDevice(c.hv.device)) != hipSuccess) return hip_fail(e);
  Stream stream;
  if ((e = hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking)) != hipSuccess) return hip_fail(e);
  BatchBuffers B[2];
  DeviceBuffer d_clicks;
  for (BatchBuffers& b : B) {
    if ((e = hipHostMalloc((void**)&b.h_blob, c.blob_cap, hipHostMallocDefault)) != hipSuccess || (e = hipMalloc(&b.d_blob.p, c.blob_cap)) != hipSuccess ||
        (e = hipMalloc(&b.d_xyzi.p, 16 * c.xyzi_cap)) != hipSuccess)
      return hip_fail(e);
    if (!(b.plan = ilcc_unpack_plan_create(c.frames_cap))) return ILCC_HIP_ERROR;
  }
  if ((e = hipMalloc(&d_clicks.p, 12ull * c.frames_cap)) != hipSuccess) return hip_fail(e);

  // the seed
  float seed[3] = {0, 0, 0};
  if (seed_mode == ILCC_SEED_CLICK) {
    std::memcpy(seed, click, 12);
  } else {
    ilcc_seed_params seedp;
    ilcc_seed_planar_params planarp;
    ilcc_params p = c.hv.p;
    if (seed_mode == ILCC_SEED_AUTO) ilcc_default_seed_params(&p, &seedp);
    else ilcc_default_seed_planar_params(&p, &seedp, &planarp);
    bool found = false;
    std::vector<float> xyzi;
    std::vector<ilcc_result> res(1);
    for (uint32_t k = 0; k < n_sel && k < ILCC_SEQUENCE_AUTO_TRIES && !found; ++k) {
      c.next_scan = k;
      c.have_pending = false;
      const uint32_t keep = c.frames_cap;
      c.frames_cap = 1;
      st = c.stage(&B[0]);
      c.frames_cap = keep;
      if (st != ILCC_OK || (st = c.upload(&B[0], stream.s)) != ILCC_OK) return st;
      const uint64_t n = B[0].points;
      if (n == 0) continue;
      xyzi.resize(4 * n);
      if ((e = hipMemcpy(xyzi.data(), B[0].d_xyzi.p, 16 * n, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail(e);
      std::memset(static_cast<void*>(res.data()), 0, sizeof(ilcc_result));
      int32_t rank = -1;
      float s3[3];
      st = seed_mode == ILCC_SEED_AUTO ? ilcc_extract_auto(h, xyzi.data(), (uint32_t)n, &seedp, res.data(), s3, &rank)
                                       : ilcc_extract_auto_planar(h, xyzi.data(), (uint32_t)n, &seedp, &planarp, res.data(), s3, &rank);
      if (st != ILCC_OK) return fail(st, std::string("seed: ") + ilcc_last_error(h));
      if (rank >= 0 && res[0].status == ILCC_OK) {
        std::memcpy(seed, s3, 12);
        found = true;
      }
    }
    c.next_scan = 0;
    c.have_pending = false;
    if (!found) return fail(ILCC_BOARD_NOT_FOUND, "no chessboard proposal was accepted on the first scans");
  }
  std::memcpy(out->click, seed, 12);
  {
    std::vector<float> clicks(3ull * c.frames_cap);
    for (uint32_t f = 0; f < c.frames_cap; ++f) std::memcpy(&clicks[3 * f], seed, 12);
    if ((e = hipMemcpy(d_clicks.p, clicks.data(), 12ull * c.frames_cap, hipMemcpyHostToDevice)) != hipSuccess) return hip_fail(e);
  }

  // the batches: while the pipeline works on batch k the host reads, inflates, stages, copies and unpacks batch k + 1
  std::vector<ilcc_result> results(n_sel);
  std::memset(static_cast<void*>(results.data()), 0, sizeof(ilcc_result) * n_sel);
  TicketInFlight flying;
  flying.h = h;
  flying.sink.resize(c.frames_cap);
  int cur = 0;
  if ((st = c.stage(&B[cur])) != ILCC_OK || (st = c.upload(&B[cur], stream.s)) != ILCC_OK) return st;
  while (B[cur].scans() > 0) {
    BatchBuffers& now = B[cur];
    st = ilcc_submit_batch_device(h, static_cast<const float*>(now.d_xyzi.p), now.offsets.data(), now.scans(), static_cast<const float*>(d_clicks.p),
                                  &flying.ticket);
    if (st != ILCC_OK) {
      flying.ticket = -1;
      return fail(st, std::string("pipeline: ") + ilcc_last_error(h));
    }
    ++out->n_batches;
    BatchBuffers& next = B[cur ^ 1];   // its previous batch has been waited for
    int32_t st_next = c.stage(&next);
    if (st_next == ILCC_OK && next.scans() > 0) st_next = c.upload(&next, stream.s);
    const int32_t ticket = flying.ticket;
    flying.ticket = -1;
    st = ilcc_wait(h, ticket, &results[now.first_scan]);
    if (st != ILCC_OK) return fail(st, std::string("pipeline: ") + ilcc_last_error(h));
    if (st_next != ILCC_OK) return st_next;
    cur ^= 1;
  }

  // acceptance and fusion
  std::vector<float> corners((size_t)n_sel * n_corners * 3);
  std::vector<uint8_t> accepted(n_sel), used(n_sel);
  std::vector<double> dist(n_sel);
  for (uint32_t s = 0; s < n_sel; ++s) {
    accepted[s] = scan_accepted(results[s], sp, n_corners) ? 1 : 0;
    std::memcpy(&corners[(size_t)s * n_corners * 3], results[s].corners, 12u * (size_t)n_corners);
  }
  const double gate = sp.gate > 0 ? sp.gate : c.hv.p.grid_length / 2;
  ilcc_fused_corners fused;
  st = ilcc_fuse_corners(corners.data(), accepted.data(), n_sel, (uint32_t)(c.hv.p.board_w - 1), (uint32_t)(c.hv.p.board_h - 1), gate, &fused, used.data(),
                         dist.data());
  out->n_ok = fused.n_ok;
  out->n_used = fused.n_used;
  out->ref_scan = fused.ref_scan;
  out->n_corners = fused.n_corners;
  out->spread_rms = fused.spread_rms;
  out->spread_max = fused.spread_max;
  std::memcpy(out->corners, fused.corners, sizeof(fused.corners));
  if (per_scan_out)
    for (uint32_t s = 0; s < n_sel; ++s) {
      records[s].result = results[s];
      records[s].accepted = accepted[s];
      records[s].used = used[s];
      records[s].distance = dist[s];
      per_scan_out[s] = records[s];
    }
  if (st == ILCC_AMBIGUOUS) return fail(st, "the accepted scans do not agree on one corner set (the board moved, or no majority within the gate)");
  if (st == ILCC_BOARD_NOT_FOUND) return fail(st, "no scan was accepted");
  if (st != ILCC_OK) return fail(st, "fusion refused its input");
  return ILCC_OK;
}

}  // namespace

extern "C" {

void ilcc_default_sequence_params(ilcc_sequence_params* sp) {
  if (!sp) return;
  std::memset(sp, 0, sizeof(*sp));
  sp->stride = 1;
  sp->staging_bytes = kDefaultStagingBytes;
}

int32_t ilcc_bag_corners_all_scans(ilcc_handle* h, const char* bag_path, const char* topic, const float* click, int32_t seed_mode,
                                   const ilcc_sequence_params* sp, ilcc_sequence_result* out, ilcc_scan_record* per_scan_out, uint32_t cap) {
  if (!out) return fail(ILCC_BAD_ARGUMENT, "null argument");
  std::memset(out, 0, sizeof(*out));
  out->ref_scan = -1;
  int32_t st;
  if (!h || !bag_path || !topic || !sp || (per_scan_out == nullptr && cap != 0)) {
    st = fail(ILCC_BAD_ARGUMENT, "null argument");
  } else if (seed_mode != ILCC_SEED_CLICK && seed_mode != ILCC_SEED_AUTO && seed_mode != ILCC_SEED_AUTO_PLANAR) {
    st = fail(ILCC_BAD_ARGUMENT, "unknown seed mode");
  } else if (seed_mode == ILCC_SEED_CLICK && !click) {
    st = fail(ILCC_BAD_ARGUMENT, "seed mode CLICK needs a click");
  } else {
    try {   // no exception crosses the C-ABI
      st = all_scans(h, bag_path, topic, click, seed_mode, *sp, out, per_scan_out, cap);
    } catch (const std::bad_alloc&) {
      st = fail(ILCC_IO_ERROR, "out of memory");
    } catch (...) {
      st = fail(ILCC_IO_ERROR, "sequence: unknown failure");
    }
  }
  out->status = st;
  return st;
}

}  // extern "C"
