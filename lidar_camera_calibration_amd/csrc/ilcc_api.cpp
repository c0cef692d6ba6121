// ilcc_api.cpp -- the handle behind the C-ABI (include/ilcc_hip.h): its HBM buffers and slots, the stage pipeline on the handle's
// three HIP streams, the one path every batch entry takes (run_batch), the waits, HIP-event timing, and the diagnostic and fetch
// entries.  What needs no handle (parameters, status texts, the two file contracts of the path) is ilcc_params.cpp.
#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "ilcc_internal.h"
#include "k15_seed.h"
#include "k6_common.h"
#include "k7_common.h"

using namespace ilcc;

namespace ilcc {
bool params_ok(const ilcc_params& p, std::string& why);   // ilcc_params.cpp
}

#ifndef ILCC_SLOTS
#define ILCC_SLOTS 4
#endif
constexpr int kSlots = ILCC_SLOTS;   // batches in flight per handle (submit/wait); slot 0 serves the synchronous calls.
                            // A slot holds buffers, events and staging, no stream: the batches share the handle's kStreams
                            // streams, so the hardware queues a handle needs do not grow with the batches in flight
constexpr int kStreams = 3;   // the handle's streams: batch seq runs whole on S[seq mod 3]

// A batch's timing events, in the order the pipeline records them (= the columns of the debug timeline behind the slot number)
enum BatchEvent {
  kEvStart,         // in front of K1
  kEvCropCounted,   // between K1's count pass and its scatter
  kEvCropped,       // behind K1
  kEvClustered,     // behind K2
  kEvPlane,         // behind K3
  kEvLabelled,      // behind K4/K5: the grid search starts here
  kEvWalkOrdered,   // behind K5w
  kEvSeeded,        // behind the seed launch (or the whole of k6_locate)
  kEvRefined,       // behind the refinement launch
  kEvAnchored,      // behind the anchor rounds
  kEvPrepassed,     // behind the common pre-pass: here the full pass may have to wait for the previous batch's
  kEvFullStart,     // in front of the full pass
  kEvSearched,      // behind the full pass (GRID mode; else = kEvLabelled's successor)
  kEvEnd,           // behind K7
  kEvCount
};
static_assert(kEvCount == ILCC_TIMELINE_COLS - 1, "a timeline row is the slot and one time per event");

// What a batch runs: the ROI pipeline (crop around the click, cluster, plane, labels, grid search or local solve, corners) or
// get_chessboard_by_point's front half (no crop: the whole cloud in two tiers, up to the labels).  A ticket carries its batch's
// kind: only ilcc_wait_chessboard_by_point applies the by-point epilogue
enum BatchKind { kRoiPipeline, kByPoint };

// One in-flight batch: its events, stage buffers and pinned result staging.
struct Slot {
  hipEvent_t ev[kEvCount]{};   // by BatchEvent (kEvWalkOrdered ... kEvFullStart: GRID batches only)
  hipEvent_t done = nullptr;   // the batch's last command (what a wait synchronises on: never a whole shared stream)
  hipEvent_t late = nullptr;   // behind what a wait enqueues itself (K9 into d_records, the late compact pack, ensure_full's copy)
  hipEvent_t k6_done = nullptr;   // no timing: behind the full pass (the next batch's full pass waits for it)
  bool allocated = false;
  // device buffers
  float4* d_xyzi = nullptr;   // staging for host-input calls
  float* d_clicks = nullptr;
  uint64_t* d_off = nullptr;
  ilcc_result* d_res = nullptr;
  float4 *d_roi = nullptr, *d_cluster = nullptr, *d_board = nullptr, *d_pca = nullptr, *d_optim = nullptr;
  float2 *d_yz = nullptr, *d_walk_yz = nullptr;
  uint8_t* d_walk_lab = nullptr;
  uint32_t *d_walk_mi = nullptr, *d_walk_nrim = nullptr;
  uint8_t *d_lab = nullptr, *d_cls = nullptr;
  uint32_t *d_nlab = nullptr, *d_walk = nullptr, *d_counts = nullptr, *d_parent = nullptr, *d_count = nullptr;
  unsigned long long* d_masks = nullptr;
  uint32_t *d_hash_head = nullptr, *d_hash_next = nullptr;
  uint32_t *d_flags = nullptr, *d_nfinite = nullptr, *d_counts_fin = nullptr;   // the online caller's two tiers (Ctx::frame_flags, n_finite, crop_fin)
  uint32_t* h_online = nullptr;   // pinned: flags then finite counts of the last online batch
  uint32_t* d_list = nullptr;     // tier 2: [0] count, [1..] listed frames
  uint32_t* d_fallback = nullptr; // K2: the frames k2_seeded_cluster hands to k2_fallback_cluster (Ctx::fallback_list; their count is a batch word)
  void* d_list_frames = nullptr;  // tier 2: kListedFrameBytes per frame
  GridPartial *d_partial = nullptr, *d_partial2 = nullptr, *d_partial3 = nullptr, *d_partial4 = nullptr;
  SolveRec* d_solverec = nullptr;
  uint32_t *d_bound = nullptr, *d_bound_sub = nullptr;
  uint32_t* d_tie_count = nullptr;
  GridPartial* d_tie_list = nullptr;
  unsigned long long* d_iters = nullptr;
  uint32_t *d_grp_alive = nullptr, *d_grp_mask = nullptr;   // K6's common pre-pass per (frame, group of kThetaGroup thetas): state word, rejected-tile mask
  size_t grp_alive_cap = 0, grp_mask_cap = 0;   // sized from (max_frames, the handle's grid) in alloc_slot / ilcc_set_params, never in the submit path
  uint32_t* d_work_list = nullptr;   // ... and the pre-pass's hand-over to the full pass (GridPass::work_list): max_frames x n_th items, sized with them
  size_t work_list_cap = 0;
  float* h_rec_dev = nullptr;               // the DEVICE address of h_rec (pinned, mapped): K9 stores the batch's compact records straight into it
  unsigned long long* h_iters_dev = nullptr;   // ... and of h_iters
  // pinned host staging
  float* h_rec = nullptr;
  ilcc_result* h_res = nullptr;
  unsigned long long* h_iters = nullptr;
  uint64_t* h_off = nullptr;   // pinned copy of `off`: the upload at the head of a batch must not stage through pageable memory
  // state of the batch in flight / last completed
  std::vector<uint64_t> off;
  uint32_t n_frames = 0;
  bool busy = false, grid = false;
  bool listed = false;       // the batch in flight / last completed ran a common pre-pass that handed over its list: h_iters[kLiveWord] is its live count
  BatchKind kind = kRoiPipeline;   // of the batch in flight
  bool h_res_valid = false;  // h_res holds the last completed batch's full (trimmed) records
  bool compact = false;      // what was enqueued with the batch in flight: the K9 records (true) or the trimmed full records
  uint32_t rec_corners = 0;  // corners per K9 record of that batch
};

struct ilcc_handle {
  int device = 0;
  ilcc_params p{};
  uint32_t max_frames = 0;
  uint64_t max_points = 0;
  uint32_t max_theta = 0;
  uint32_t crop_chunks_cap = 0;
  Slot slots[kSlots];
  hipStream_t stream[kStreams]{};   // S0, S1, S2: created with the handle, shared by the slots
  uint64_t seq = 0;     // batches enqueued so far: batch seq takes S[seq mod 3]
  uint64_t stream_last[kStreams]{};   // per stream, 1 + seq of the last batch enqueued on it (0: none yet)
  hipEvent_t entry_done = nullptr;    // no timing: behind the work of a diagnostic entry or a table upload
  int next_slot = 0;    // round robin for ilcc_submit_*
  int last_slot = -1;   // slot whose batch the fetch calls look at
  int k6_last = -1;     // slot that issued the most recent full pass (full passes are chained: they never share the chip)
  // candidate tables (shared by all slots, read-only while batches are in flight)
  float *d_cth = nullptr, *d_sth = nullptr, *d_ay = nullptr, *d_az = nullptr;
  // decimated subset of the same tables: seeding pass of K6's branch and bound
  float *d_cth2 = nullptr, *d_sth2 = nullptr, *d_ay2 = nullptr, *d_az2 = nullptr;
  // what the kernels are given of them (upload_tables): the full grid, the seed grid, and where the seed's entries sit in the full one
  GridTables grid{}, seed_grid{};
  SeedMap seed_map{2, 12, 6};
  // K7r: cos/sin of the theta lattice (grid step / refine_div, refine_th_margin grid steps beyond the grid on both sides)
  double2* d_th_lattice = nullptr;
  size_t th_lattice_cap = 0;
  int32_t th_lat_lo = 0, th_lat_hi = 0, hop_y = 0, hop_z = 0;
  double* d_solve = nullptr;   // 3 theta_t + 2 (cost, iterations) for the test entries
  RefineOut* d_refine_io = nullptr;
  uint32_t grid_lds_points = 1024;   // grows with the frames seen (grow_capacities); frames above it take the global-memory path
  uint64_t group_prepass_skipped = 0;   // batches whose grid was eligible for k6_group_prepass but whose mask buffers were too small: a sizing bug if ever non-zero -- the first such batch leaves a note in ilcc_last_error (results are unaffected: the full pass runs without the common mask)
  uint32_t cluster_lds_points = 2048;   // K2's LDS capacity for cell-sorted ROI points per frame: grows likewise (<= 4096); larger frames sort into HBM
  uint32_t cluster_cells_cap = kClusterCellsMin;   // K2's LDS capacity in occupied cells per frame: grows with what the batches needed
  uint32_t list_grid = 1024;         // workgroups of the online caller's second-tier kernels (4 x the device's CUs)
  bool poisoned = false;             // a failed ilcc_set_params could not restore the device tables: every later call fails
  int32_t result_mode = ILCC_RESULTS_FULL;
  ilcc_timing timing{};
  hipEvent_t tl_ref = nullptr;       // ilcc_debug_timeline_*: reference event, rows of ILCC_TIMELINE_COLS doubles
  bool tl_on = false;
  // The full pass's launch form (enqueue_grid_search).  live_hist: the live (frame, theta) workgroups per frame, in 1/65536, of the
  // last kLiveHist completed batches that listed them (finish) -- a rate, so that a batch of another size can use it
  int32_t full_pass_mode = ILCC_FULL_PASS_RULE;   // ilcc_debug_full_pass_launch
  uint32_t full_pass_forced_g = 0;                // ILCC_FULL_PASS_LISTED: its workgroups
  static constexpr int kLiveHist = 8;
  uint64_t live_hist[kLiveHist]{};
  int live_hist_n = 0, live_hist_at = 0;
  uint32_t full_pass_last[ILCC_FULL_PASS_LAST_WORDS]{};   // ilcc_debug_full_pass_last
  bool separate_launches = false;    // ilcc_debug_separate_launches: K3, K4/K5, K5w and K1's two kernels as launches of their own at any batch size
  ClusterLimits cluster_limits{};    // K2's residency limits on this device (launch_cluster's rule for the home of the sorted points)
  int32_t cluster_home = kClusterHomeRule;   // ilcc_debug_cluster_home: the rule, or one home forced
  ClusterLaunch cluster_last{};      // what the last k2_seeded_cluster launch used (ilcc_debug_cluster_launch)
  uint32_t cluster_fallback_last = 0;   // frames of the last finished batch that k2_seeded_cluster handed to k2_fallback_cluster (likewise)
  std::vector<double> tl_rows;
  std::string err;
};

namespace {

thread_local std::string g_err;

#define HIP_TRY(h, expr)                                                                   \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess) {                                                                \
      (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                        \
      return ILCC_HIP_ERROR;                                                               \
    }                                                                                      \
  } while (0)

// ... and a step of the library's own that failed has said why already
#define ILCC_TRY(expr)                   \
  do {                                   \
    const int32_t st_ = (expr);          \
    if (st_ != ILCC_OK) return st_;      \
  } while (0)

int32_t near_zero_index(double vmin, double step, int32_t n) {
  long c = std::lround(-vmin / step);
  if (c < 0) c = 0;
  if (c > n - 1) c = n - 1;
  return (int32_t)c;
}

// a diagnostic entry or a table upload waits for its own work on an event behind it, never for the whole shared stream
int32_t sync_own(ilcc_handle* h, hipStream_t s) {
  HIP_TRY(h, hipEventRecord(h->entry_done, s));
  HIP_TRY(h, hipEventSynchronize(h->entry_done));
  return ILCC_OK;
}

// (only where no batch is in flight: a whole shared stream also holds the later batches)
int32_t sync_all(ilcc_handle* h) {
  for (hipStream_t s : h->stream)
    if (s) HIP_TRY(h, hipStreamSynchronize(s));
  return ILCC_OK;
}

int32_t upload_tables(ilcc_handle* h) {
  const ilcc_params& p = h->p;
  if ((uint32_t)p.n_th > h->max_theta || (uint32_t)p.n_ty > h->max_theta || (uint32_t)p.n_tz > h->max_theta) {
    h->err = "grid axis longer than the handle's table capacity";
    return ILCC_CAPACITY;
  }
  hipStream_t st = h->stream[0];
  std::vector<float> cth(p.n_th), sth(p.n_th), ay(p.n_ty), az(p.n_tz);
  const double g = p.grid_length;
  for (int k = 0; k < p.n_th; ++k) {
    const double th = p.th_min + k * p.th_step;
    cth[k] = (float)(std::cos(th) / g);
    sth[k] = (float)(std::sin(th) / g);
  }
  for (int a = 0; a < p.n_ty; ++a) ay[a] = (float)(((p.ty_min + a * p.ty_step) + p.board_w * g / 2.0) / g);
  for (int b = 0; b < p.n_tz; ++b) az[b] = (float)(((p.tz_min + b * p.tz_step) + p.board_h * g / 2.0) / g);
  HIP_TRY(h, hipMemcpyAsync(h->d_cth, cth.data(), sizeof(float) * p.n_th, hipMemcpyHostToDevice, st));
  HIP_TRY(h, hipMemcpyAsync(h->d_sth, sth.data(), sizeof(float) * p.n_th, hipMemcpyHostToDevice, st));
  HIP_TRY(h, hipMemcpyAsync(h->d_ay, ay.data(), sizeof(float) * p.n_ty, hipMemcpyHostToDevice, st));
  HIP_TRY(h, hipMemcpyAsync(h->d_az, az.data(), sizeof(float) * p.n_tz, hipMemcpyHostToDevice, st));
  // seed subset: ~5 thetas (centred, so theta = 0 is one of them for a symmetric grid) x 8 x 8 translations --
  // the same float values as the full tables.  The seed only has to land in the right basin: the refinement
  // pass then evaluates everything around its argmin (theta +- half a seed stride, 8 x 8 translations), which
  // on the synthetic VLP-16 set yields the exact grid minimum as the bound in 46 of 46 frames (seed alone:
  // 3-20 x the minimum).  Measured on the 128-frame batch (K6 ms): translation stride 2: 1.05, 4: 0.91, 5: 0.83.
#ifndef ILCC_SEED_THETAS
#define ILCC_SEED_THETAS 5
#endif
#ifndef ILCC_REFINE_RADIUS_DIV
#define ILCC_REFINE_RADIUS_DIV 3   // refinement pass: theta radius = seed stride / 3 (measured in the pipelined bench: /2: 245.3 k, /3: 248.9 k, /4: 245.6 k frames/s)
#endif
  SeedMap& map = h->seed_map;
  map.stride_th = std::max(2, p.n_th / ILCC_SEED_THETAS);
  map.stride_t = std::max(1, std::min(p.n_ty, p.n_tz) / 8);
  map.off_th = map.stride_th / 2;
  std::vector<float> cth2, sth2, ay2, az2;
  for (int k = map.off_th; k < p.n_th; k += map.stride_th) {
    cth2.push_back(cth[k]);
    sth2.push_back(sth[k]);
  }
  for (int a = 0; a < p.n_ty; a += map.stride_t) ay2.push_back(ay[a]);
  for (int b = 0; b < p.n_tz; b += map.stride_t) az2.push_back(az[b]);
  // the "nearest to zero" indices: each grid's own (a kernel reads ay[c_ty] / az[c_tz] and uses all three for the tie-break distance)
  GridTables& full = h->grid;
  full = GridTables{h->d_cth, h->d_sth, h->d_ay, h->d_az, p.n_th, p.n_ty, p.n_tz, near_zero_index(p.th_min, p.th_step, p.n_th),
                    near_zero_index(p.ty_min, p.ty_step, p.n_ty), near_zero_index(p.tz_min, p.tz_step, p.n_tz)};
  GridTables& seed = h->seed_grid;
  seed = GridTables{h->d_cth2, h->d_sth2, h->d_ay2, h->d_az2, (int32_t)cth2.size(), (int32_t)ay2.size(), (int32_t)az2.size(), 0, 0, 0};
  seed.c_th = std::min(std::max(full.c_th / map.stride_th, 0), seed.n_th - 1);
  seed.c_ty = std::min(full.c_ty / map.stride_t, seed.n_ty - 1);
  seed.c_tz = std::min(full.c_tz / map.stride_t, seed.n_tz - 1);
  if (seed.n_th > 0) {
    HIP_TRY(h, hipMemcpyAsync(h->d_cth2, cth2.data(), sizeof(float) * cth2.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(h->d_sth2, sth2.data(), sizeof(float) * sth2.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(h->d_ay2, ay2.data(), sizeof(float) * ay2.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(h->d_az2, az2.data(), sizeof(float) * az2.size(), hipMemcpyHostToDevice, st));
  }
  // K7r: cos/sin of every theta lattice point, from the host's libm -- the oracle evaluates cos()/sin() of the
  // SAME doubles (th_min + q * (th_step / div)) with the same libm, so the kernel's per-point terms are the oracle's
  {
    const int div = p.refine_div > 0 ? p.refine_div : 1;
    h->th_lat_lo = -p.refine_th_margin * div;
    h->th_lat_hi = (p.n_th - 1 + p.refine_th_margin) * div;
    const size_t n = (size_t)(h->th_lat_hi - h->th_lat_lo) + 1;
    if (n > h->th_lattice_cap) {
      if (h->d_th_lattice) (void)hipFree(h->d_th_lattice);
      h->d_th_lattice = nullptr;
      h->th_lattice_cap = 0;
      HIP_TRY(h, hipMalloc((void**)&h->d_th_lattice, sizeof(double2) * n));
      h->th_lattice_cap = n;
    }
    std::vector<double2> tab(n);
    for (size_t i = 0; i < n; ++i) {
      const double th = p.th_min + (double)(h->th_lat_lo + (int64_t)i) * (p.th_step / (double)div);
      tab[i] = make_double2(std::cos(th), std::sin(th));
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_th_lattice, tab.data(), sizeof(double2) * n, hipMemcpyHostToDevice, st));
    const int32_t sst = sync_own(h, st);   // tab is a local
    if (sst != ILCC_OK) return sst;
    h->hop_y = (int32_t)std::lround(p.grid_length / (p.ty_step / (double)div));
    h->hop_z = (int32_t)std::lround(p.grid_length / (p.tz_step / (double)div));
  }
  return sync_own(h, st);
}

// The handle's buffers, and a slot's buffers and events, are each named ONCE: in the lists that both the allocation and the release walk
struct Buffer {
  void** ptr;
  size_t bytes;   // 0: sized elsewhere, released with the rest
};
template <class T>
Buffer buffer(T*& p, size_t count) { return {reinterpret_cast<void**>(&p), sizeof(T) * count}; }

auto handle_buffers(ilcc_handle* h) {
  const size_t mt = h->max_theta;
  return std::array{buffer(h->d_cth, mt),  buffer(h->d_sth, mt),  buffer(h->d_ay, mt),  buffer(h->d_az, mt),
                    buffer(h->d_cth2, mt), buffer(h->d_sth2, mt), buffer(h->d_ay2, mt), buffer(h->d_az2, mt),
                    buffer(h->d_solve, 8), buffer(h->d_refine_io, 1), buffer(h->d_th_lattice, 0) /* follows the grid: upload_tables */};
}

auto slot_device_buffers(const ilcc_handle* h, Slot& sl) {
  const size_t np = h->max_points, mf = h->max_frames, chunks = h->crop_chunks_cap, mt = h->max_theta;
  return std::array{
      buffer(sl.d_xyzi, np),
      buffer(sl.d_clicks, 3 * mf),
      buffer(sl.d_off, mf + 1),
      buffer(sl.d_res, mf),
      buffer(sl.d_roi, np),
      buffer(sl.d_cluster, np),
      buffer(sl.d_board, np),
      buffer(sl.d_pca, np),
      buffer(sl.d_optim, np),
      buffer(sl.d_yz, np),
      buffer(sl.d_walk_yz, np),
      buffer(sl.d_walk_lab, np),
      buffer(sl.d_walk_mi, mf),
      buffer(sl.d_walk_nrim, mf),
      buffer(sl.d_lab, np),
      buffer(sl.d_cls, np),
      buffer(sl.d_nlab, mf),
      buffer(sl.d_walk, mf),
      buffer(sl.d_counts, chunks),
      buffer(sl.d_counts_fin, chunks),
      buffer(sl.d_flags, mf),
      buffer(sl.d_nfinite, mf),
      buffer(sl.d_list, mf + 1),
      buffer(sl.d_fallback, mf),
      Buffer{&sl.d_list_frames, kListedFrameBytes * mf},
      buffer(sl.d_masks, chunks * (kCropChunk / 64)),
      buffer(sl.d_parent, np),
      buffer(sl.d_count, np),
      buffer(sl.d_hash_head, mf * kClusterHashSize),
      buffer(sl.d_hash_next, np),
      buffer(sl.d_partial, mf * mt),
      buffer(sl.d_partial2, mf * mt),
      buffer(sl.d_partial3, mf * mt),
      buffer(sl.d_partial4, mf * 4),
      buffer(sl.d_solverec, 2 * mf),
      buffer(sl.d_bound, mf),
      buffer(sl.d_bound_sub, mf),
      buffer(sl.d_tie_count, mf),
      buffer(sl.d_tie_list, mf * kTieCap),
      buffer(sl.d_iters, kBatchWords),
      buffer(sl.d_grp_alive, 0),   // the common pre-pass's two follow the grid: size_group_prepass
      buffer(sl.d_grp_mask, 0),
      buffer(sl.d_work_list, 0),
  };
}

auto slot_pinned_buffers(const ilcc_handle* h, Slot& sl) {
  const size_t mf = h->max_frames;
  return std::array{
      buffer(sl.h_res, mf),
      buffer(sl.h_rec, mf * (ILCC_RECORD_HEADER + 3 * ILCC_MAX_CORNERS)),
      buffer(sl.h_iters, kBatchWords),
      buffer(sl.h_off, mf + 1),
      buffer(sl.h_online, 2 * mf),
  };
}

struct SlotEvent {
  hipEvent_t* ev;
  unsigned flags;
};
auto slot_events(Slot& sl) {
  std::array<SlotEvent, kEvCount + 3> evs;
  for (int k = 0; k < kEvCount; ++k) evs[k] = {&sl.ev[k], hipEventDefault};   // the batch's timing events
  evs[kEvCount] = {&sl.done, hipEventDisableTiming};
  evs[kEvCount + 1] = {&sl.late, hipEventDisableTiming};
  evs[kEvCount + 2] = {&sl.k6_done, hipEventDisableTiming};
  return evs;
}

// (also of a slot whose allocation stopped half-way: whatever the lists hold is released, the slot is as new)
void free_slot(const ilcc_handle* h, Slot& sl) {
  for (const Buffer& b : slot_device_buffers(h, sl))
    if (*b.ptr) (void)hipFree(*b.ptr);
  for (const Buffer& b : slot_pinned_buffers(h, sl))
    if (*b.ptr) (void)hipHostFree(*b.ptr);
  for (const SlotEvent& e : slot_events(sl))
    if (*e.ev) (void)hipEventDestroy(*e.ev);
  sl = Slot{};
}

// The HIP runtime maps streams onto the hardware queues GPU_MAX_HW_QUEUES allows, and streams that share a queue
// serialise.  A handle's three streams plus the host's own stream need 4 queues, HIP's default.  The variable is read when
// the runtime initialises and belongs to the HOST process: the library only reads it, and says so once when it is below 4.
void warn_hw_queues_once() {
  static std::once_flag once;   // handles of several threads (one per GPU) may reach this together
  std::call_once(once, [] {
    const char* v = std::getenv("GPU_MAX_HW_QUEUES");
    if (!v || std::atoi(v) >= kStreams + 1) return;
    std::fprintf(stderr,
                 "libilcc_hip: GPU_MAX_HW_QUEUES=%s: with fewer than %d hardware queues two of the handle's stage streams "
                 "(or one and the host's stream) share a queue and serialise (the library does not modify the "
                 "environment)\n", v, kStreams + 1);
  });
}

// K6's common pre-pass: does the handle's grid qualify, and what its output needs per frame
struct GroupPrepassPlan {
  bool box = false;   // the grid is eligible for the box pre-passes at all (the ONE place that decides it)
  bool on = false;
  uint32_t groups = 0, words = 0;   // theta groups per frame = ceil(n_th / kThetaGroup); mask words per group = ceil(tiles / 32)
};
GroupPrepassPlan group_prepass_plan(const ilcc_params& p) {
  GroupPrepassPlan g;
  // box pre-pass (k6_common.h: box_term): its monotonicity argument needs a tile's box narrower than one square on both axes
  const bool box = p.grid_prune != 0 && 3.0 * p.ty_step < 0.9 * p.grid_length && 3.0 * p.tz_step < 0.9 * p.grid_length;
  // ... and, for the points the common pre-pass leaves out, every translation of the tables keeping the board's centre inside the board
  const double gl = p.grid_length;
  const double ty_hi = p.ty_min + (p.n_ty - 1) * p.ty_step, tz_hi = p.tz_min + (p.n_tz - 1) * p.tz_step;
  const bool centre_in = p.ty_min > -0.45 * p.board_w * gl && ty_hi < 0.45 * p.board_w * gl && p.tz_min > -0.45 * p.board_h * gl &&
                         tz_hi < 0.45 * p.board_h * gl;
  const uint32_t n_tiles = (uint32_t)grid_tiles(p.n_ty, p.n_tz);
  g.box = box;
  g.on = box && p.n_th >= kThetaGroup && centre_in && n_tiles <= (uint32_t)kBoxTilesMax;
  g.groups = (uint32_t)((p.n_th + kThetaGroup - 1) / kThetaGroup);
  g.words = (n_tiles + 31u) / 32u;
  return g;
}

// (re)size a slot's common pre-pass buffers for the handle's current grid.  hipFree synchronises the device, so this runs
// where no batch can be in flight: alloc_slot (a slot's first use) and ilcc_set_params -- never inside a submit.
int32_t size_group_prepass(ilcc_handle* h, Slot& sl) {
  const GroupPrepassPlan g = group_prepass_plan(h->p);
  if (!g.on) return ILCC_OK;
  const size_t need_alive = (size_t)h->max_frames * g.groups, need_mask = need_alive * g.words;
  if (need_alive > sl.grp_alive_cap) {
    if (sl.d_grp_alive) (void)hipFree(sl.d_grp_alive);
    sl.d_grp_alive = nullptr;
    sl.grp_alive_cap = 0;
    HIP_TRY(h, hipMalloc((void**)&sl.d_grp_alive, sizeof(uint32_t) * need_alive));
    sl.grp_alive_cap = need_alive;
  }
  if (need_mask > sl.grp_mask_cap) {
    if (sl.d_grp_mask) (void)hipFree(sl.d_grp_mask);
    sl.d_grp_mask = nullptr;
    sl.grp_mask_cap = 0;
    HIP_TRY(h, hipMalloc((void**)&sl.d_grp_mask, sizeof(uint32_t) * need_mask));
    sl.grp_mask_cap = need_mask;
  }
  const size_t need_list = (size_t)h->max_frames * (size_t)h->p.n_th;   // one item per (frame, theta): every workgroup of the full pass alive
  if (need_list > sl.work_list_cap && need_list <= 0xFFFFFFFFull) {     // (an item is a 32-bit record index; a larger batch keeps the (n_th, F) launch)
    if (sl.d_work_list) (void)hipFree(sl.d_work_list);
    sl.d_work_list = nullptr;
    sl.work_list_cap = 0;
    HIP_TRY(h, hipMalloc((void**)&sl.d_work_list, sizeof(uint32_t) * need_list));
    sl.work_list_cap = need_list;
  }
  return ILCC_OK;
}

// ---- The full pass's launch form.  k6_group_prepass lists the live (frame, theta) workgroups (GridPass::work_list); the listed
// launch starts G workgroups for them instead of n_th x n_frames of which most return at once.  The host cannot know the count of
// the batch it is enqueueing without a synchronisation, so G comes from the batches that have completed: the live share is a
// property of the data (how well the locate launches bound a frame), steady from batch to batch.  Correctness never depends on
// G: items beyond G are run by the looping launch behind the listed one, workgroups beyond the count find nothing to do.
//   observed < 0: no batch has come back yet -> the (n_th, F) launch.
//   G = observed + 1/4 + 64, rounded up to a multiple of 256 (the device's compute units), within [1, n_th x n_frames].  The margin
//   is wide on measurement: workgroups that find no item cost nothing that shows, items beyond G wait for the
//   second, looping launch (G at 3/4 of the count: the full pass + 40 %).
//   G above 3/4 of the full grid: the (n_th, F) launch -- with nearly every workgroup alive the listed launch measured 1.2 % SLOWER
//   (669 -> 677 us), with a third alive 4-7 % faster; the two lines cross at 70-80 %.
// Returns the form; *workgroups = G (what the listed form would start, also when the rule does not take it).
int32_t full_pass_rule(int64_t observed, uint32_t n_th, uint32_t n_frames, uint32_t* workgroups) {
  const uint64_t full = (uint64_t)n_th * n_frames;
  uint64_t g = full;
  if (observed >= 0) {
    const uint64_t o = (uint64_t)observed;
    g = (o + o / 4u + 64u + 255u) & ~(uint64_t)255u;
  }
  g = std::max<uint64_t>(1u, std::min<uint64_t>(g, std::min<uint64_t>(full, 0x7FFFFFFFull)));
  *workgroups = (uint32_t)g;
  return observed >= 0 && full > 0 && g * 4u <= full * 3u ? ILCC_FULL_PASS_LISTED : ILCC_FULL_PASS_GRID;
}

// the live workgroups a batch of n_frames is expected to list: the largest rate among the handle's recently completed batches (-1: none)
int64_t expected_live(const ilcc_handle* h, uint32_t n_frames) {
  if (h->live_hist_n == 0) return -1;
  uint64_t rate = 0;
  for (int k = 0; k < h->live_hist_n; ++k) rate = std::max(rate, h->live_hist[k]);
  return (int64_t)((rate * n_frames + 65535u) >> 16);
}
void note_live(ilcc_handle* h, uint64_t live, uint32_t n_frames) {
  if (n_frames == 0) return;
  h->live_hist[h->live_hist_at] = ((live << 16) + n_frames - 1u) / n_frames;
  h->live_hist_at = (h->live_hist_at + 1) % ilcc_handle::kLiveHist;
  h->live_hist_n = std::min(h->live_hist_n + 1, (int)ilcc_handle::kLiveHist);
}

int32_t alloc_slot_parts(ilcc_handle* h, Slot& sl) {
  for (const SlotEvent& e : slot_events(sl)) HIP_TRY(h, hipEventCreateWithFlags(e.ev, e.flags));
  for (const Buffer& b : slot_device_buffers(h, sl))
    if (b.bytes) HIP_TRY(h, hipMalloc(b.ptr, b.bytes));
  for (const Buffer& b : slot_pinned_buffers(h, sl)) HIP_TRY(h, hipHostMalloc(b.ptr, b.bytes, hipHostMallocDefault));
  // (the records and counters are written by kernels, not by D2H copies: the device's view of the two pinned buffers)
  HIP_TRY(h, hipHostGetDevicePointer((void**)&sl.h_rec_dev, sl.h_rec, 0));
  HIP_TRY(h, hipHostGetDevicePointer((void**)&sl.h_iters_dev, sl.h_iters, 0));
  return size_group_prepass(h, sl);
}

// A slot's first use.  A failure half-way releases what the slot had got, so the next use of the slot starts over
int32_t alloc_slot(ilcc_handle* h, Slot& sl) {
  if (sl.allocated) return ILCC_OK;
  const int32_t st = alloc_slot_parts(h, sl);
  if (st != ILCC_OK) {
    free_slot(h, sl);
    return st;
  }
  sl.allocated = true;
  return ILCC_OK;
}

Ctx make_ctx(ilcc_handle* h, Slot& sl, const float4* d_xyzi, const float* d_clicks, uint32_t n_frames,
             uint32_t crop_chunks) {
  Ctx c{};
  c.xyzi = d_xyzi;
  c.off = sl.d_off;
  c.clicks = d_clicks;
  c.n_frames = n_frames;
  c.crop_chunks = crop_chunks;
  c.res = sl.d_res;
  c.roi = sl.d_roi;
  c.cluster = sl.d_cluster;
  c.board = sl.d_board;
  c.pca = sl.d_pca;
  c.optim = sl.d_optim;
  c.yz = sl.d_yz;
  c.lab = sl.d_lab;
  c.cls = sl.d_cls;
  c.n_lab = sl.d_nlab;
  c.walk_stride = sl.d_walk;
  c.walk_yz = sl.d_walk_yz;
  c.walk_lab = sl.d_walk_lab;
  c.walk_mi = sl.d_walk_mi;
  c.walk_nrim = sl.d_walk_nrim;
  c.crop_counts = sl.d_counts;
  c.crop_masks = sl.d_masks;
  c.uf_parent = sl.d_parent;
  c.uf_count = sl.d_count;
  c.uf_hash_head = sl.d_hash_head;
  c.uf_hash_next = sl.d_hash_next;
  c.cluster_lds_points = h->cluster_lds_points;
  c.cluster_cells_cap = h->cluster_cells_cap;
  c.wide = 0u;
  c.cluster_bits = cluster_bits_default();
  c.fallback_list = sl.d_fallback;
  c.online_tier = 0u;
  c.online_window = 0.f;
  c.frame_flags = sl.d_flags;
  c.n_finite = sl.d_nfinite;
  c.crop_fin = sl.d_counts_fin;
  c.list_count = sl.d_list;
  c.list = sl.d_list + 1;
  c.list_frames = sl.d_list_frames;
  c.list_grid = h->list_grid;
  c.partial = sl.d_partial;
  c.solve_rec = sl.d_solverec;
  c.grid_blocks = (uint32_t)h->p.n_th;
  c.grid_lds_points = h->grid_lds_points;
  c.grid_bound = sl.d_bound;
  c.grid_bound_sub = sl.d_bound_sub;
  c.tie_count = sl.d_tie_count;
  c.tie_list = sl.d_tie_list;
  c.grid_iters = sl.d_iters;
  c.grid = h->grid;
  c.th_lattice = h->d_th_lattice;
  c.th_lat_lo = h->th_lat_lo;
  c.th_lat_hi = h->th_lat_hi;
  c.refine_hop_y = h->hop_y;
  c.refine_hop_z = h->hop_z;
  c.p = h->p;
  return c;
}

int32_t check_offsets(ilcc_handle* h, const uint64_t* offsets, uint32_t n_frames) {
  if (!offsets || n_frames == 0) {
    h->err = "no frames";
    return ILCC_BAD_ARGUMENT;
  }
  if (n_frames > h->max_frames) {
    h->err = "n_frames exceeds the handle's max_frames";
    return ILCC_CAPACITY;
  }
  if (offsets[0] != 0) {
    h->err = "offsets[0] must be 0";
    return ILCC_BAD_ARGUMENT;
  }
  for (uint32_t f = 0; f < n_frames; ++f)
    if (offsets[f + 1] < offsets[f] || offsets[f + 1] - offsets[f] > 0x7FFFFFFFull) {
      h->err = "offsets must be non-decreasing, frames < 2^31 points";
      return ILCC_BAD_ARGUMENT;
    }
  if (offsets[n_frames] > h->max_points) {
    h->err = "total points exceed the handle's max_total_points";
    return ILCC_CAPACITY;
  }
  return ILCC_OK;
}

// The next batch's stream: batch seq runs whole on S[seq mod 3]
int take_stream(ilcc_handle* h) {
  const int k = (int)(h->seq % kStreams);
  h->stream_last[k] = ++h->seq;
  return k;
}

// Where a wait launches what it needs once its batch is complete (K9 into d_records, the late compact pack, ensure_full's copy):
// the stream whose last batch is the oldest.  A stream that holds no batch submitted after the waited one is idle.  With four
// batches in flight on three streams every stream holds a later batch, and the launch waits for the rest of the oldest of them
// (its chain wait, for the batch just finished, is already met; a younger one may still wait for full passes before it).
hipStream_t late_stream(const ilcc_handle* h) {
  int best = 0;
  for (int k = 1; k < kStreams; ++k)
    if (h->stream_last[k] < h->stream_last[best]) best = k;
  return h->stream[best];
}

// K2's workgroup keeps bitmap + per-cell arrays + (up to cluster_lds_points) sorted points in LDS: when the cell arrays have
// grown large (dense clouds), give up LDS points first -- frames of that size sort into HBM anyway
void fit_cluster_lds(ilcc_handle* h) {
  while (cluster_lds_bytes(h->cluster_lds_points, h->cluster_cells_cap, cluster_bits_online()) > (size_t)kClusterLdsMax && h->cluster_lds_points > 0)
    h->cluster_lds_points = h->cluster_lds_points > 512u ? h->cluster_lds_points - 512u : 0u;
}

uint32_t board_corners(const ilcc_params& p) { return (uint32_t)((p.board_w - 1) * (p.board_h - 1)); }
size_t trimmed_bytes(uint32_t n_corners) { return offsetof(ilcc_result, corners) + sizeof(float) * 3 * (size_t)n_corners; }

// per frame only the record's head and the board's corners (a pitched copy: rows of trimmed_bytes out of sizeof(ilcc_result))
hipError_t copy_results_trimmed(ilcc_result* dst, const ilcc_result* d_src, uint32_t n_frames, uint32_t n_corners, hipStream_t s) {
  if (n_frames == 0) return hipSuccess;
  return hipMemcpy2DAsync(dst, sizeof(ilcc_result), d_src, sizeof(ilcc_result), trimmed_bytes(n_corners), n_frames,
                          hipMemcpyDeviceToHost, s);
}

// Host-side constants of the grid search.  (A/B builds override the #defines with -D, tools/build_variant.sh; what each was
// measured at is recorded in DESIGN.md section 4 "K6" and profiles/README.md.)
#ifndef ILCC_SEED_POINTS
#define ILCC_SEED_POINTS 128   // seed and refinement walk a PREFIX of the frame's walk: a sixteenth of its labelled points (kSeedShift), at least this many
#endif
#ifndef ILCC_BOX_POINTS
#define ILCC_BOX_POINTS 48     // rim points a (frame, theta) workgroup's own box pre-pass looks at, at least
#endif
constexpr int kAnchorRadius = 1;   // the anchor scores 2 * 1 + 1 thetas around the refinement's argmin, one 4 x 4 tile each, on ALL points
#ifndef ILCC_ANCHOR_ROUNDS
#define ILCC_ANCHOR_ROUNDS 2
#endif
constexpr int kAnchorRounds = ILCC_ANCHOR_ROUNDS;   // k6_anchor rounds, each re-centred on the previous one's argmin (config 5: 62.5 -> 70.6 k frames/s)

// ---- The launches of the grid search, one GridPass each.  whole_grid_pass is the plain evaluation; every other constructor starts
// from it and names only what its launch differs in.

// every candidate of `t` on every labelled point, one workgroup per theta, following no other launch, against the frame's bound:
// what ilcc_grid_cost runs
GridPass whole_grid_pass(const Ctx& c, const GridTables& t, GridPartial* out) {
  GridPass g{};
  g.t = t;
  g.out = out;
  g.blocks = (uint32_t)t.n_th;
  g.bound = c.grid_bound;
  return g;
}

// `blocks` records per frame from a launch over the FULL tables
GridSeed full_table_records(const GridPartial* records, uint32_t blocks) { return GridSeed{records, blocks, SeedMap{1, 1, 0}}; }

// seed: the decimated tables on a prefix of the walk.  Sums over a prefix are not costs of complete candidates: a bound word of their own
GridPass seed_pass(const ilcc_handle* h, const Slot& sl, const Ctx& c) {
  GridPass g = whole_grid_pass(c, h->seed_grid, sl.d_partial2);
  g.walk_limit = (uint32_t)ILCC_SEED_POINTS;
  g.bound = c.grid_bound_sub;
  return g;
}

// refinement: every kRefineThetaStride-th theta within refine_radius steps of the seed's argmin, a window of translations that
// spans the seed's stride around it; the same prefix of the walk and bound word as the seed
GridPass refine_pass(const ilcc_handle* h, const Slot& sl, const Ctx& c, int32_t refine_radius) {
  GridPass g = whole_grid_pass(c, h->grid, sl.d_partial3);
  g.seed = GridSeed{sl.d_partial2, (uint32_t)h->seed_grid.n_th, h->seed_map};
  g.window_tiles = h->seed_map.stride_t > 2 * kTile ? 4 : 2;
  g.radius_th = (refine_radius / kRefineThetaStride) * kRefineThetaStride;
  g.step_th = kRefineThetaStride;
  g.blocks = std::min((uint32_t)(2 * (g.radius_th / kRefineThetaStride) + 1), h->max_theta);
  g.walk_limit = (uint32_t)ILCC_SEED_POINTS;
  g.bound = c.grid_bound_sub;
  return g;
}

// one anchor round (k6_anchor): 2 kAnchorRadius + 1 thetas x one tile around the argmin of `seed`, on ALL points -- complete costs,
// which publish the frame's real bound
GridPass anchor_pass(const ilcc_handle* h, const Ctx& c, const GridSeed& seed, GridPartial* out) {
  GridPass g = whole_grid_pass(c, h->grid, out);
  g.seed = seed;
  g.radius_th = kAnchorRadius;
  g.blocks = 2 * kAnchorRadius + 1;
  return g;
}

// full pass: the whole grid behind the bound the launches before it published (seed: their records, its starting tile; none on a
// grid too small to locate on), collecting the near ties for K7r.  The box pre-passes are set by enqueue_grid_search
GridPass full_pass(const ilcc_handle* h, const Ctx& c, const GridSeed& seed) {
  GridPass g = whole_grid_pass(c, h->grid, c.partial);
  g.seed = seed;
  g.collect_ties = 1u;
  return g;
}

// k6_locate's plan: the handle's two grids, the sample, one record per frame
LocatePlan locate_plan(const ilcc_handle* h, const Slot& sl, const Ctx& c) {
  LocatePlan lp{};
  lp.seed = h->seed_grid;
  lp.map = h->seed_map;
  lp.refine_radius = std::max(1, h->seed_map.stride_th / ILCC_REFINE_RADIUS_DIV);
  lp.sample_min = (uint32_t)ILCC_SEED_POINTS;
  lp.sample_cap = std::max((uint32_t)ILCC_SEED_POINTS, ((c.grid_lds_points >> 3) + 63u) & ~63u);
  lp.stage_cap = ILCC_LOCATE_STAGE_ANCHOR ? c.grid_lds_points : 0u;
  lp.out = sl.d_partial4;
  return lp;
}

// How a batch of n_frames locates the minimum in front of the full pass: not at all (a grid too small to decimate), with the three
// kinds of launches, or in one launch, one workgroup per frame (k6_locate), when the batch has the frames to fill the chip that way
// and the plan's LDS fits.  The values are what ilcc_debug_grid_solve_batch reports.
enum LocateForm { kLocateNone = 0, kLocateLaunches = 1, kLocateFused = 2 };
LocateForm locate_form(const ilcc_handle* h, const LocatePlan& lp, uint32_t n_frames) {
  if (!(h->seed_grid.n_th > 0 && h->p.n_th >= 8 && h->p.n_ty >= 8 && h->p.n_tz >= 8)) return kLocateNone;
  const bool fused = n_frames >= (uint32_t)kLocateMinFrames && lp.seed.n_th <= 16 &&
                     locate_lds_bytes(lp, h->grid.n_ty, h->grid.n_tz) <= (size_t)kLocateLdsMax;
  return fused ? kLocateFused : kLocateLaunches;
}

// Locating the minimum with three kinds of launches (batches too small for k6_locate's one workgroup per frame): seed over the
// decimated tables, refinement around its argmin, then kAnchorRounds anchor rounds, each re-centred on the previous round's argmin
// -- a greedy descent on complete costs towards the grid minimum, for a tighter bound in front of the full pass.  Returns where
// the full pass finds the last round's records.
int32_t enqueue_locate_launches(ilcc_handle* h, Slot& sl, const Ctx& c, hipStream_t s, int32_t refine_radius, GridSeed& located) {
  launch_grid_cost(c, seed_pass(h, sl, c), s, /*use_oob=*/1, nullptr, true);
  HIP_TRY(h, hipEventRecord(sl.ev[kEvSeeded], s));
  const GridPass refine = refine_pass(h, sl, c, refine_radius);
  launch_grid_cost(c, refine, s, /*use_oob=*/1, nullptr, true);
  HIP_TRY(h, hipEventRecord(sl.ev[kEvRefined], s));
  located = full_table_records(refine.out, refine.blocks);
  GridPartial* const ping[2] = {sl.d_partial4, sl.d_partial2};
  for (int round = 0; round < kAnchorRounds; ++round) {
    const GridPass anchor = anchor_pass(h, c, located, ping[round & 1]);
    launch_anchor(c, anchor, s);
    located = full_table_records(anchor.out, anchor.blocks);
  }
  return ILCC_OK;
}

// The grid search of one batch: K5w (walk layout), the launches that locate the minimum and publish the frame's bound (k6_locate,
// or seed + refinement + anchor rounds), the common pre-pass, the full pass -- with the slot's K6 events recorded in between.
// chain: the full pass waits for the previous batch's, on whichever stream that one runs (every batch; the diagnostic entry
// ilcc_grid_solve runs alone).
// walk_laid_out: the front end's one launch has written the walk layout already.
int32_t enqueue_grid_search(ilcc_handle* h, Slot& sl, const Ctx& c, hipStream_t s, uint32_t n_frames, bool chain, bool walk_laid_out = false) {
  const bool prune = h->p.grid_prune != 0;
  if (!walk_laid_out) launch_walk_order(c, s);   // K5w: the labelled points in K6's walk layout, once per frame
  HIP_TRY(h, hipEventRecord(sl.ev[kEvWalkOrdered], s));
  GridSeed located{};   // (records == nullptr: nothing located)
  // (grid_prune = 0 keeps the locate launches: they only initialise the frame's bound, which the cut-free full
  // pass still needs to recognise near ties; it never cuts a tile)
  const LocatePlan lp = locate_plan(h, sl, c);
  const LocateForm located_by = locate_form(h, lp, n_frames);
  if (located_by != kLocateNone) {
    // These launches only have to LOCATE the minimum.  Seed and refinement therefore look at a prefix of the point walk (an
    // eighth of the frame's labelled points, at least ILCC_SEED_POINTS positions: a uniform sample of the board) and keep their
    // own bound word; the anchor evaluates what they found on EVERY point and publishes the frame's real bound.  (Round 2 ran
    // seed and refinement on all points: 16 % of the path's VALU instructions.)
    if (located_by == kLocateFused) {
      launch_locate(c, s, lp);
      HIP_TRY(h, hipEventRecord(sl.ev[kEvSeeded], s));   // (the whole locate launch is accounted as the "seed" span)
      HIP_TRY(h, hipEventRecord(sl.ev[kEvRefined], s));
      located = full_table_records(lp.out, 1);
    } else {
      ILCC_TRY(enqueue_locate_launches(h, sl, c, s, lp.refine_radius, located));
    }
  } else {
    HIP_TRY(h, hipEventRecord(sl.ev[kEvSeeded], s));
    HIP_TRY(h, hipEventRecord(sl.ev[kEvRefined], s));
  }
  HIP_TRY(h, hipEventRecord(sl.ev[kEvAnchored], s));   // behind the anchor: the common pre-pass gets an event span of its own
  GridPass full = full_pass(h, c, located);
  const GroupPrepassPlan gp = group_prepass_plan(h->p);
  full.box_points = gp.box ? (uint32_t)ILCC_BOX_POINTS : 0u;   // (eligibility: group_prepass_plan, which also sized the buffers)
  // k6_group_prepass: one box pre-pass for kThetaGroup consecutive thetas, launched HERE -- behind the anchor (it needs the
  // frame's bound), in front of the full pass.  Its buffers were sized for (max_frames, this grid) by alloc_slot / ilcc_set_params.
  if (full.box_points != 0u && gp.on && (size_t)n_frames * gp.groups <= sl.grp_alive_cap &&
      (size_t)n_frames * gp.groups * gp.words <= sl.grp_mask_cap) {
    full.grp_alive = sl.d_grp_alive;
    full.grp_mask = sl.d_grp_mask;
    full.grp_count = gp.groups;
    full.grp_words = gp.words;
    if ((size_t)n_frames * full.blocks <= sl.work_list_cap) {   // (sized with the masks)
      full.work_list = sl.d_work_list;
      full.work_count = reinterpret_cast<uint32_t*>(c.grid_iters + kLiveWord);   // (little-endian: the word's low half; K1 / the diagnostic entries reset it)
    }
    launch_group_prepass(c, full, s);
  } else if (full.box_points != 0u && gp.on) {
    // eligible grid, buffers too small for this batch (never expected: size_group_prepass sized them): slower, not wrong -- say so once
    if (h->group_prepass_skipped++ == 0) h->err = "note: k6_group_prepass skipped (mask buffers smaller than this batch needs): slower, results unaffected";
  }
  HIP_TRY(h, hipEventRecord(sl.ev[kEvPrepassed], s));
  // The FULL passes of consecutive batches are chained so that they never share the chip (two passes side by side both run at
  // half speed and every batch's front end waits longer for wave slots); the launches above are small and are left free to
  // overlap with another batch's full pass, like K2 / K3 / K7.
  const int si = (int)(&sl - h->slots);
  if (chain && h->k6_last >= 0 && h->k6_last != si && h->slots[h->k6_last].busy)
    HIP_TRY(h, hipStreamWaitEvent(s, h->slots[h->k6_last].k6_done, 0));
  HIP_TRY(h, hipEventRecord(sl.ev[kEvFullStart], s));
  // the listed launch needs the hand-over and is the pruning full pass; every other full pass keeps the (n_th, F) launch
  uint32_t g = 0;
  int32_t form = full_pass_rule(expected_live(h, n_frames), full.blocks, n_frames, &g);
  if (h->full_pass_mode == ILCC_FULL_PASS_GRID) form = ILCC_FULL_PASS_GRID;
  if (h->full_pass_mode == ILCC_FULL_PASS_LISTED) {
    form = ILCC_FULL_PASS_LISTED;
    g = std::min(h->full_pass_forced_g, full.blocks * n_frames);
  }
  if (full.work_list == nullptr || !prune || n_frames == 0) form = ILCC_FULL_PASS_GRID;
  sl.listed = full.work_list != nullptr;
  if (form == ILCC_FULL_PASS_LISTED)
    launch_grid_cost_listed(c, full, s, g);
  else
    launch_grid_cost(c, full, s, /*use_oob=*/1, nullptr, prune);
  h->full_pass_last[0] = (uint32_t)form;
  h->full_pass_last[1] = form == ILCC_FULL_PASS_LISTED ? g : full.blocks * n_frames;
  if (chain) {
    HIP_TRY(h, hipEventRecord(sl.k6_done, s));
    h->k6_last = si;
  }
  return ILCC_OK;
}

int32_t enqueue_impl(ilcc_handle* h, int si, hipStream_t s, const float4* d_xyzi, const uint64_t* offsets, uint32_t n_frames,
                     const float* d_clicks, BatchKind kind) {
  Slot& sl = h->slots[si];
  uint64_t max_n = 0;
  for (uint32_t f = 0; f < n_frames; ++f) max_n = std::max<uint64_t>(max_n, offsets[f + 1] - offsets[f]);
  uint32_t chunks = (uint32_t)((max_n + kCropChunk - 1) / kCropChunk);
  if (chunks == 0) chunks = 1;
  if ((uint64_t)chunks * n_frames > (uint64_t)h->crop_chunks_cap) {
    h->err = "crop chunk table too small for this (very ragged) batch";
    return ILCC_CAPACITY;
  }
  sl.off.assign(offsets, offsets + n_frames + 1);
  sl.n_frames = n_frames;
  std::memcpy(sl.h_off, sl.off.data(), sizeof(uint64_t) * (n_frames + 1));
  HIP_TRY(h, hipMemcpyAsync(sl.d_off, sl.h_off, sizeof(uint64_t) * (n_frames + 1), hipMemcpyHostToDevice, s));
  // (result records, component counters, K6 counters and near-tie counters are reset inside K1 / K2)
  Ctx c = make_ctx(h, sl, d_xyzi, d_clicks, n_frames, chunks);
  HIP_TRY(h, hipEventRecord(sl.ev[kEvStart], s));
  if (kind == kRoiPipeline) {
    // (one pass, one workgroup per frame, when the batch has the frames for it)
    launch_roi_crop(c, s, sl.ev[kEvCropCounted], !h->separate_launches && n_frames >= (uint32_t)kCropFrameMinFrames);
    HIP_TRY(h, hipEventRecord(sl.ev[kEvCropped], s));
    h->cluster_last = launch_cluster(c, s, h->cluster_limits, h->cluster_home);
  } else {
    // get_chessboard_by_point clusters the WHOLE cloud (no ROI; setClusterTolerance(0.1), LidarCornersEst.cpp:80 -- EuclideanCluster()
    // uses 0.12, :131) and keeps the cluster around the predicted point.  Two tiers, identical results:
    //   1. K1 crops a +-1.25 m window around the point, K2 clusters it on the LDS cell grid -- the ROI pipeline's fast path -- and
    //      verifies that the whole cloud gives the same cluster (fine_cluster_frame: nearest point, admissible, complete);
    //   2. the frames it could not vouch for: K1 with an unbounded box (only non-finite points go), K2 on hashed cells.
    c.p.cluster_tol = c.p.online_cluster_tol;
    c.wide = 1u;   // a synchronous call: latency is all that counts
    Ctx t1 = c;
    t1.online_tier = 1u;
    t1.online_window = 1.25f;
    t1.p.roi_half[0] = t1.p.roi_half[1] = t1.p.roi_half[2] = (double)t1.online_window;
    t1.cluster_bits = cluster_bits_online();
    launch_roi_crop(t1, s, sl.ev[kEvCropCounted]);
    HIP_TRY(h, hipEventRecord(sl.ev[kEvCropped], s));
    h->cluster_last = launch_cluster(t1, s, h->cluster_limits, h->cluster_home);
    Ctx t2 = c;
    t2.online_tier = 2u;
    t2.p.roi_half[0] = t2.p.roi_half[1] = t2.p.roi_half[2] = (double)INFINITY;
    launch_roi_crop(t2, s, nullptr);
    launch_cluster_listed(t2, s);
    HIP_TRY(h, hipMemcpyAsync(sl.h_online, sl.d_flags, sizeof(uint32_t) * n_frames, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(sl.h_online + h->max_frames, sl.d_nfinite, sizeof(uint32_t) * n_frames, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(h, hipEventRecord(sl.ev[kEvClustered], s));
  sl.grid = kind == kRoiPipeline && h->p.solver == ILCC_SOLVER_GRID;
  // K3, K4/K5 and (GRID mode) K5w: one launch when the batch would run them at the same width anyway.  The whole launch is then
  // accounted as the K3 span, like k6_locate as the seed's
  const bool one_launch = !h->separate_launches && front_end_fusable(c);
  if (one_launch) {
    launch_front_end(c, s, /*walk_layout=*/sl.grid);
    HIP_TRY(h, hipEventRecord(sl.ev[kEvPlane], s));
  } else {
    launch_ransac_plane(c, s);
    HIP_TRY(h, hipEventRecord(sl.ev[kEvPlane], s));
    launch_plane_frame_hist(c, s);
  }
  HIP_TRY(h, hipEventRecord(sl.ev[kEvLabelled], s));
  if (sl.grid) {
    ILCC_TRY(enqueue_grid_search(h, sl, c, s, n_frames, /*chain=*/true, /*walk_laid_out=*/one_launch));
  }
  HIP_TRY(h, hipEventRecord(sl.ev[kEvSearched], s));
  if (kind == kRoiPipeline) {
    if (sl.grid) {
      launch_pattern_refine(c, s);   // (with the near ties of the full pass, re-ordered on fixed-point sums by K7r)
    } else {
      launch_reference_solve(c, s);
    }
    launch_corners(c, s, solve_slots(c.p));
  }
  HIP_TRY(h, hipEventRecord(sl.ev[kEvEnd], s));
  HIP_TRY(h, hipGetLastError());
  // the copy back: what the result mode asks for rides on the batch's stream (include/ilcc_hip.h, "Result traffic")
  sl.compact = h->result_mode == ILCC_RESULTS_COMPACT;
  sl.rec_corners = board_corners(h->p);
  // (compact records and the batch counters are STORED into the pinned staging by kernels: no D2H command in the SDMA queue that
  // carries the next batches' input copies -- launch_store_to_host)
  if (sl.compact) {
    launch_pack_records(sl.d_res, n_frames, sl.rec_corners, 0u, sl.h_rec_dev, s);   // K9 writes the records straight into the pinned staging
  } else {
    HIP_TRY(h, copy_results_trimmed(sl.h_res, sl.d_res, n_frames, sl.rec_corners, s));
  }
  launch_store_to_host(sl.d_iters, sl.h_iters_dev, sizeof(unsigned long long) * kBatchWords, s);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipEventRecord(sl.done, s));
  sl.busy = true;
  sl.kind = kind;
  return ILCC_OK;
}

// enqueue the whole path for one batch on the stream (no host synchronisation).  On a mid-pipeline failure the kernels already
// queued may still be running on the slot's buffers: wait for them before handing the error back, so that the next submit can
// reuse the slot.  (The batch is the newest one: its stream holds nothing behind it.)
int32_t enqueue(ilcc_handle* h, int si, hipStream_t s, const float4* d_xyzi, const uint64_t* offsets, uint32_t n_frames,
                const float* d_clicks, BatchKind kind) {
  if (h->poisoned) {
    h->err = "handle unusable: a failed ilcc_set_params could not restore the device tables";
    return ILCC_HIP_ERROR;
  }
  const int32_t st = enqueue_impl(h, si, s, d_xyzi, offsets, n_frames, d_clicks, kind);
  if (st != ILCC_OK) {
    const std::string why = h->err;
    (void)hipStreamSynchronize(s);
    (void)hipGetLastError();
    h->slots[si].busy = false;
    h->err = why;
  }
  return st;
}

// What a wait launches for a batch that has completed (on late_stream) is waited for on its own event
int32_t run_late(ilcc_handle* h, Slot& sl, hipStream_t s) {
  HIP_TRY(h, hipEventRecord(sl.late, s));
  HIP_TRY(h, hipEventSynchronize(sl.late));
  return ILCC_OK;
}

// the slot's full records in its pinned staging (they are there already unless the batch ran in ILCC_RESULTS_COMPACT mode)
int32_t ensure_full(ilcc_handle* h, Slot& sl) {
  if (sl.h_res_valid) return ILCC_OK;
  const hipStream_t s = late_stream(h);
  HIP_TRY(h, copy_results_trimmed(sl.h_res, sl.d_res, sl.n_frames, sl.rec_corners, s));
  ILCC_TRY(run_late(h, sl, s));
  sl.h_res_valid = true;
  return ILCC_OK;
}

// ---- A wait in four parts: wait_batch, hand_over, account_timing, grow_capacities (finish runs them in turn)

// wait for the slot's batch, then launch and wait for what this wait wants beyond what was enqueued with the batch: K9 into
// d_records, the compact records of a batch submitted in ILCC_RESULTS_FULL mode
int32_t wait_batch(ilcc_handle* h, Slot& sl, bool want_compact, float* d_records, uint32_t n_corners, uint32_t tag_base) {
  HIP_TRY(h, hipSetDevice(h->device));   // (a wait may come from another thread than the submit)
  HIP_TRY(h, hipEventSynchronize(sl.done));
  const bool pack_now = want_compact && !sl.compact;   // the compact records were not enqueued with the batch
  const hipStream_t ls = late_stream(h);
  if (d_records) launch_pack_records(sl.d_res, sl.n_frames, n_corners, tag_base, d_records, ls);
  if (pack_now) launch_pack_records(sl.d_res, sl.n_frames, sl.rec_corners, 0u, sl.h_rec_dev, ls);
  if (d_records || pack_now) {
    ILCC_TRY(run_late(h, sl, ls));
  }
  sl.busy = false;
  sl.h_res_valid = !sl.compact;
  h->last_slot = (int)(&sl - h->slots);
  return ILCC_OK;
}

size_t record_floats(const Slot& sl) { return (size_t)ILCC_RECORD_HEADER + 3 * (size_t)sl.rec_corners; }

// hand the completed batch's records to the caller: full and / or compact
int32_t hand_over(ilcc_handle* h, Slot& sl, ilcc_result* out, float* out_compact) {
  if (out) {
    ILCC_TRY(ensure_full(h, sl));
    const size_t row = trimmed_bytes(sl.rec_corners);
    for (uint32_t f = 0; f < sl.n_frames; ++f) std::memcpy(&out[f], &sl.h_res[f], row);
  }
  if (out_compact) std::memcpy(out_compact, sl.h_rec, sizeof(float) * sl.n_frames * record_floats(sl));
  return ILCC_OK;
}

// what the completed batch's records say about its frames
struct BatchCounts {
  uint32_t max_lab = 0, max_roi = 0;   // the most labelled points of a frame that reached the search; the most ROI points K2's LDS path can hold
  uint64_t evals = 0;                  // (labelled point, candidate) pairs of the whole grid
};
BatchCounts count_batch(const ilcc_handle* h, const Slot& sl) {
  BatchCounts n;
  for (uint32_t f = 0; f < sl.n_frames; ++f) {
    // (status, n_roi, labelled points) from whichever record came back with the batch
    int32_t status, n_roi;
    uint32_t m;
    if (sl.h_res_valid) {
      const ilcc_result& r = sl.h_res[f];
      status = r.status;
      n_roi = r.n_roi;
      m = (uint32_t)(r.n_black + r.n_white);
    } else {
      const float* r = sl.h_rec + (size_t)f * record_floats(sl);
      status = (int32_t)r[0];
      n_roi = (int32_t)r[19];
      m = (uint32_t)r[13] + (uint32_t)r[14];
    }
    if (n_roi > 0 && (uint32_t)n_roi <= (uint32_t)kClusterLdsPointsMax) n.max_roi = std::max(n.max_roi, (uint32_t)n_roi);
    if (status != ILCC_OK && status != ILCC_AMBIGUOUS) continue;
    n.max_lab = std::max(n.max_lab, m);
    n.evals += (uint64_t)m * (uint64_t)h->p.n_th * h->p.n_ty * h->p.n_tz;
  }
  return n;
}

// the batch's events into ilcc_timing (and the debug timeline)
int32_t account_timing(ilcc_handle* h, const Slot& sl, uint64_t evals) {
  auto span = [&](BatchEvent from, BatchEvent to, float& ms_out) { return hipEventElapsedTime(&ms_out, sl.ev[from], sl.ev[to]); };
  float ms[6];   // K1, K2, K3, K4/K5, K6, K7: from one of these events to the next
  const BatchEvent stage[7] = {kEvStart, kEvCropped, kEvClustered, kEvPlane, kEvLabelled, kEvSearched, kEvEnd};
  for (int k = 0; k < 6; ++k) HIP_TRY(h, span(stage[k], stage[k + 1], ms[k]));
  float k6k[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // K5w, seed, refinement, anchor, common pre-pass; full pass
  if (sl.grid) {   // K6 = (what locates the minimum + the common pre-pass) + (full pass); the wait for the previous batch's full pass in between is not K6 time
    const BatchEvent part[6] = {kEvLabelled, kEvWalkOrdered, kEvSeeded, kEvRefined, kEvAnchored, kEvPrepassed};
    for (int k = 0; k < 5; ++k) HIP_TRY(h, span(part[k], part[k + 1], k6k[k]));
    HIP_TRY(h, span(kEvFullStart, kEvSearched, k6k[5]));
    float pre = 0.f;
    HIP_TRY(h, span(kEvLabelled, kEvPrepassed, pre));
    ms[4] = pre + k6k[5];
  }
  float tot = 0;
  HIP_TRY(h, span(kEvStart, kEvEnd, tot));
  if (h->tl_on && h->tl_ref && sl.grid) {
    h->tl_rows.push_back((double)(&sl - h->slots));
    for (hipEvent_t e : sl.ev) {   // (BatchEvent order = the timeline's columns)
      float t = 0.f;
      HIP_TRY(h, hipEventElapsedTime(&t, h->tl_ref, e));
      h->tl_rows.push_back((double)t);
    }
  }
  ilcc_timing& t = h->timing;
  t.roi_crop = ms[0];
  t.cluster = ms[1];
  t.ransac_plane = ms[2];
  t.plane_frame_hist = ms[3];
  t.grid_cost = ms[4];
  t.refine_corners = ms[5];
  t.total = tot;
  t.batches += 1;
  for (int k = 0; k < 6; ++k) t.stage_ms_sum[k] += ms[k];
  t.stage_ms_sum[6] += tot;
  {
    float cnt = 0.f;
    HIP_TRY(h, span(kEvStart, kEvCropCounted, cnt));
    t.roi_count_ms_sum += cnt;
  }
  if (sl.grid) {
    t.grid_cost_launches += 1;
    t.grid_cost_ms_sum += ms[4];
    t.walk_order_ms_sum += k6k[0];
    t.grid_cost_kernel_ms_sum += (double)k6k[1] + k6k[2] + k6k[3] + k6k[4] + k6k[5];
    t.grid_cost_locate_ms_sum += (double)k6k[1] + k6k[2] + k6k[3];
    t.grid_cost_prepass_ms_sum += k6k[4];
    t.grid_cost_full_ms_sum += k6k[5];
    t.grid_cost_evals_nominal_sum += evals;
    // (both colour phases of a (point, candidate) pair = 1 evaluation)
    unsigned long long iters = 0;
    unsigned long long iters_in = 0;
    for (int k = 0; k < kIterSlots; ++k) {
      iters += sl.h_iters[k];
      iters_in += sl.h_iters[kIterSlots + k];
      t.grid_cost_box_evals_sum += sl.h_iters[2 * kIterSlots + k];
    }
    t.grid_cost_evals_sum += (uint64_t)iters * grid_cost_evals_per_count();
    t.grid_cost_evals_interior_sum += (uint64_t)iters_in * grid_cost_evals_per_count();
  }
  return ILCC_OK;
}

// An LDS capacity for frames that need `need` entries: rounded up to `step` (a power of two), within [lo, hi].  The one rule
// behind both the growth with the frames seen and ilcc_reserve
uint32_t lds_capacity(uint32_t need, uint32_t step, uint32_t lo, uint32_t hi) {
  return std::min(hi, std::max(lo, (need + step - 1u) & ~(step - 1u)));
}
uint32_t grid_lds_capacity(uint32_t labelled_points) { return lds_capacity(labelled_points, 256u, 1024u, (uint32_t)kGridLdsPointsMax); }
uint32_t cluster_lds_capacity(uint32_t roi_points, uint32_t lo) { return lds_capacity(roi_points, 512u, lo, (uint32_t)kClusterLdsPointsMax); }
uint32_t cluster_cells_capacity(uint64_t cells) {
  const uint32_t need = (uint32_t)std::min<uint64_t>(cells, (uint64_t)kClusterCellsMax);
  return lds_capacity(need, 256u, (uint32_t)kClusterCellsMin, (uint32_t)kClusterCellsMax);
}
void raise_capacities(ilcc_handle* h, uint32_t grid_points, uint32_t cluster_points, uint32_t cluster_cells) {
  h->grid_lds_points = std::max(h->grid_lds_points, grid_points);
  h->cluster_lds_points = std::max(h->cluster_lds_points, cluster_points);
  h->cluster_cells_cap = std::max(h->cluster_cells_cap, cluster_cells);
  fit_cluster_lds(h);
}

// Adapt the three LDS capacities to what the frames of a batch needed (later calls).
// K6 / K7 staging: the largest labelled-point count so far, rounded up to 256 points.  (Not to a power of two: 1 781 points -- the
// largest of the bench frames -- need 21.8 KB per K6 workgroup at 1 792 and 24.9 KB at 2 048: seven instead of six workgroups per
// CU -- which, the kernel being VALU-bound, measured no difference: 248.8 k vs 250 k frames/s.)
// ... but never, on its own, past the capacity at which TWO workgroups of the K6 full pass still share a CU (grid_points_two_per_cu:
// 6 400 points for both BASELINE grids).  Round 6: a stream of 64-ring
// frames whose closest boards hold 6 682 labelled points (the first 128 frames: 6 170) grew the staging to 6 912 points, ONE
// workgroup per CU, and every frame's full pass took 1.15 ms instead of 0.74 ms per 128 frames.  The few frames above the capacity
// walk their points through L2 (grid_cost_body<LDS_POINTS = false>); ilcc_reserve may still ask for more, explicitly.
// K2's one-workgroup LDS path likewise (ROI points per frame, steps of 512): what it does not hold of a CU's 160 KiB is room for K6
// workgroups of other batches.  Its per-cell arrays: the most occupied cells a frame of the batch needed (+ 1/8), steps of 256.
// Frames the LDS cell grid cannot hold at any capacity (bounding grid too large: un-cropped clouds; more cells than the largest
// capacity) take the hashed-cell path in the fallback launch (k2_fallback.hip, k2_hashed.h).
constexpr int kGridStaticLds = 3072;   // static LDS of a full-pass workgroup (bests, counters, the box pre-pass's mask and list), rounded up
// the largest multiple of 256 staged points with which two full-pass workgroups on an n_ty x n_tz grid fit a CU's LDS (0: none)
constexpr uint32_t grid_points_two_per_cu(int n_ty, int n_tz) {
  const int64_t room = (int64_t)kCuLdsBytes / 2 - kGridStaticLds - (int64_t)grid_lds_bytes(0, n_ty, n_tz);
  return room > 0 ? (uint32_t)(room / (int64_t)grid_lds_bytes(1, 0, 0)) & ~255u : 0u;
}
static_assert(grid_points_two_per_cu(40, 40) == 6400, "BASELINE config 2 (the default grid: 40 x 40 translations)");
static_assert(grid_points_two_per_cu(129, 129) == 6400, "BASELINE config 5 (129 x 129 translations)");
void grow_capacities(ilcc_handle* h, const BatchCounts& n, uint64_t cells_needed) {
  const uint32_t two_per_cu = grid_points_two_per_cu(h->p.n_ty, h->p.n_tz);
  raise_capacities(h, std::min(grid_lds_capacity(n.max_lab), std::max(1024u, two_per_cu)), cluster_lds_capacity(n.max_roi, 0u),
                   cluster_cells_capacity(cells_needed + cells_needed / 8));
}

// wait for the slot's batch, hand the records over (full and / or compact), account the timing, grow the capacities
int32_t finish(ilcc_handle* h, Slot& sl, ilcc_result* out, float* out_compact = nullptr, float* d_records = nullptr,
               uint32_t n_corners = 0, uint32_t tag_base = 0) {
  ILCC_TRY(wait_batch(h, sl, out_compact != nullptr, d_records, n_corners, tag_base));
  ILCC_TRY(hand_over(h, sl, out, out_compact));
  const BatchCounts n = count_batch(h, sl);
  ILCC_TRY(account_timing(h, sl, n.evals));
  grow_capacities(h, n, sl.h_iters[3 * kIterSlots]);
  h->cluster_fallback_last = (uint32_t)sl.h_iters[kFallbackWord];
  if (sl.grid && sl.listed) {   // the batch's live count came back with its counters: the next submits size their full pass by it
    note_live(h, sl.h_iters[kLiveWord], sl.n_frames);
    h->full_pass_last[2] = (uint32_t)sl.h_iters[kLiveWord];
    h->full_pass_last[3] = sl.n_frames;
  }
  return ILCC_OK;
}

// ---- The one path of the six batch entries.  They differ in the batch's kind, in whether the input is in HBM already, and in
// whether the caller wants a ticket (the next slot in turn; all of them busy: ILCC_CAPACITY) or the records at once (slot 0, which
// ilcc_create allocated; busy: ILCC_BAD_ARGUMENT).  No hipMalloc / hipFree runs here except on a slot's first use.
int32_t run_batch(ilcc_handle* h, BatchKind kind, bool on_device, const float* xyzi, const uint64_t* offsets, uint32_t n_frames,
                  const float* clicks, int32_t* ticket, ilcc_result* out) {
  HIP_TRY(h, hipSetDevice(h->device));
  ILCC_TRY(check_offsets(h, offsets, n_frames));
  const int si = ticket ? h->next_slot : 0;
  Slot& sl = h->slots[si];
  if (sl.busy) {
    h->err = ticket ? "every pipeline slot holds a batch: wait for the oldest ticket first" : "synchronous call while ticket 0 is in flight";
    return ticket ? ILCC_CAPACITY : ILCC_BAD_ARGUMENT;
  }
  if (ticket) ILCC_TRY(alloc_slot(h, sl));
  const hipStream_t s = h->stream[take_stream(h)];
  if (!on_device) {
    // the copy rides on the batch's stream: ordered before this batch's K1, concurrent with the other batches' kernels
    if (offsets[n_frames] > 0)
      HIP_TRY(h, hipMemcpyAsync(sl.d_xyzi, xyzi, sizeof(float4) * offsets[n_frames], hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(sl.d_clicks, clicks, sizeof(float) * 3 * n_frames, hipMemcpyHostToDevice, s));
    xyzi = reinterpret_cast<const float*>(sl.d_xyzi);
    clicks = sl.d_clicks;
  }
  ILCC_TRY(enqueue(h, si, s, reinterpret_cast<const float4*>(xyzi), offsets, n_frames, clicks, kind));
  if (!ticket) return finish(h, sl, out);
  *ticket = si;
  h->next_slot = (si + 1) % kSlots;
  return ILCC_OK;
}

// ---- Tickets

const Slot* busy_slot(const ilcc_handle* h, int32_t ticket) {
  return h && ticket >= 0 && ticket < kSlots && h->slots[ticket].busy ? &h->slots[ticket] : nullptr;
}

// The slot a wait of the `kind` call family (`fn`) is to finish, or null with the reason in ilcc_last_error; the batch stays in
// flight.  A ticket belongs to the call family that issued it: ilcc_submit_chessboard_by_point's batches skip the
// crop and the search, and only their own wait applies the by-point epilogue (plane >= min_plane_points, whole-cloud n_roi); the
// other way round that epilogue would read staging no copy of the batch has filled.
Slot* ticket_slot(ilcc_handle* h, int32_t ticket, const char* fn, BatchKind kind, bool args_ok) {
  if (!h) return nullptr;
  Slot* sl = const_cast<Slot*>(busy_slot(h, ticket));
  if (!args_ok || !sl) {
    h->err = std::string(fn) + ": bad argument or no batch in flight under this ticket";
    return nullptr;
  }
  if (sl->kind != kind) {
    h->err = std::string(fn) + (sl->kind == kByPoint ? ": this ticket came from ilcc_submit_chessboard_by_point: wait with ilcc_wait_chessboard_by_point"
                                                     : ": this ticket came from ilcc_submit_batch[_device]: wait with ilcc_wait / ilcc_wait_compact / ilcc_wait_records_device");
    return nullptr;
  }
  return sl;
}

// the parameter set, the capacities and the modes belong to the batches in flight
bool any_batch_in_flight(ilcc_handle* h, const char* fn) {
  for (const Slot& sl : h->slots)
    if (sl.busy) {
      h->err = std::string(fn) + " with a batch in flight: ilcc_wait first";
      return true;
    }
  return false;
}

// what get_chessboard_by_point reports beyond the front half's record: n_roi of the WHOLE cloud, the second-tier count, and
// `if(outcloud->size() < 500 || find_board == false) return false;` (LidarCornersEst.cpp:111-112)
void finish_chessboard_by_point(ilcc_handle* h, Slot& sl, uint32_t n_frames, int32_t min_plane_points, ilcc_result* out) {
  // frames the first tier answered from a window of the cloud: n_roi is what the clustering of the WHOLE cloud runs on -- its
  // finite points (K1 counted them on the way); the handle's own copy keeps the window's count, which is what ILCC_CLOUD_ROI holds
  for (uint32_t f = 0; f < n_frames; ++f)
    if (sl.h_online[f] == 0u && out[f].status != ILCC_NO_ROI_POINTS) out[f].n_roi = (int32_t)sl.h_online[h->max_frames + f];
  for (uint32_t f = 0; f < n_frames; ++f) h->timing.online_second_tier_frames += sl.h_online[f] != 0u ? 1u : 0u;
  for (uint32_t f = 0; f < n_frames; ++f)
    if (out[f].status == ILCC_OK && (out[f].n_plane < min_plane_points || !out[f].found_board)) {
      out[f].status = ILCC_BOARD_NOT_FOUND;
      sl.h_res[f].status = ILCC_BOARD_NOT_FOUND;
    }
}

// ---- Diagnostic and fetch entries

// The slot the fetch entries read -- the last completed batch, of which they want `n` frames from `first` -- on the handle's device
int32_t fetch_slot(ilcc_handle* h, uint32_t first, uint32_t n, Slot*& slot) {
  if (!h || h->last_slot < 0) return ILCC_BAD_ARGUMENT;
  Slot& sl = h->slots[h->last_slot];
  if (sl.busy || first > sl.n_frames || n > sl.n_frames - first) {
    h->err = "fetch: no completed batch, or the frames asked for exceed it";
    return ILCC_BAD_ARGUMENT;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  slot = &sl;
  return ILCC_OK;
}

// what ilcc_fetch_labelled / ilcc_fetch_walk return: the frame's n points, of which the caller's buffers take cap_points at most
int64_t fetch_labelled_points(const float2* d_yz, const uint8_t* d_lab, uint32_t n, float* out_yz, uint8_t* out_label, uint64_t cap_points) {
  const uint64_t m = std::min<uint64_t>(n, cap_points);
  if (m > 0 && ((out_yz && hipMemcpy(out_yz, d_yz, sizeof(float2) * m, hipMemcpyDeviceToHost) != hipSuccess) ||
                (out_label && hipMemcpy(out_label, d_lab, m, hipMemcpyDeviceToHost) != hipSuccess)))
    return -(int64_t)ILCC_HIP_ERROR;
  return (int64_t)n;
}

// shared setup for the two single-kernel test entries: frame 0 of slot 0 = caller's labelled points
int32_t stage_labelled(ilcc_handle* h, hipStream_t s, const float* yz, const uint8_t* label, uint32_t m) {
  if (!h || (m > 0 && (!yz || !label))) return ILCC_BAD_ARGUMENT;
  if (m > h->max_points) {
    h->err = "more points than the handle holds";
    return ILCC_CAPACITY;
  }
  Slot& sl = h->slots[0];
  if (sl.busy) {
    h->err = "diagnostic entry while ticket 0 is in flight";
    return ILCC_BAD_ARGUMENT;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  const uint64_t off[2] = {0, m};
  ilcc_result r;
  std::memset(&r, 0, sizeof(r));
  r.status = ILCC_OK;
  HIP_TRY(h, hipMemcpyAsync(sl.d_off, off, sizeof(off), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_res, &r, sizeof(r), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_nlab, &m, sizeof(m), hipMemcpyHostToDevice, s));
  const uint32_t stride = walk_stride(m);
  HIP_TRY(h, hipMemcpyAsync(sl.d_walk, &stride, sizeof(stride), hipMemcpyHostToDevice, s));
  if (m > 0) {
    HIP_TRY(h, hipMemcpyAsync(sl.d_yz, yz, sizeof(float2) * m, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(sl.d_lab, label, m, hipMemcpyHostToDevice, s));
  }
  ILCC_TRY(sync_own(h, s));
  sl.n_frames = 0;   // the stage buffers no longer describe a batch
  return ILCC_OK;
}

// The one-frame Ctx of a diagnostic entry on slot 0, its LDS staging sized for m labelled points (m = 0: as the handle has it)
Ctx diagnostic_ctx(ilcc_handle* h, Slot& sl, uint32_t m) {
  Ctx c = make_ctx(h, sl, nullptr, nullptr, 1, 1);
  uint32_t lds = 1024;
  while (lds < m && lds < (uint32_t)kGridLdsPointsMax) lds <<= 1;
  c.grid_lds_points = std::max(c.grid_lds_points, lds);
  return c;
}

}  // namespace

namespace ilcc {
// text behind ilcc_last_error(NULL) for the handle-less entry points in other translation units
void set_global_error(const std::string& s) { g_err = s; }
// what the seed entries (seed_api.cpp) need of a handle
HandleView handle_view(const ilcc_handle* h) { return HandleView{h->device, h->p, h->max_frames, h->max_points}; }
int32_t handle_fail(ilcc_handle* h, int32_t code, const std::string& what) {
  h->err = what;
  return code;
}
}  // namespace ilcc

extern "C" {

const char* ilcc_last_error(const ilcc_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

ilcc_handle* ilcc_create(int32_t device, const ilcc_params* p, uint32_t max_frames, uint64_t max_total_points) {
  g_err.clear();
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    g_err = "no HIP device: libilcc_hip has no CPU fallback";
    return nullptr;
  }
  if (!p || max_frames == 0 || max_total_points == 0) {
    g_err = "bad arguments to ilcc_create";
    return nullptr;
  }
  std::string why;
  if (!params_ok(*p, why)) {
    g_err = why;
    return nullptr;
  }
  ilcc_handle* h = new (std::nothrow) ilcc_handle();
  if (!h) return nullptr;
  h->p = *p;
  h->max_frames = max_frames;
  h->max_points = max_total_points;
  h->max_theta = 4096;
  h->crop_chunks_cap =
      (uint32_t)std::min<uint64_t>(0xFFFFFFFFull, max_total_points / kCropChunk + (uint64_t)max_frames + 1);
  auto fail = [&](const std::string& what) {
    g_err = what;
    ilcc_destroy(h);
    return (ilcc_handle*)nullptr;
  };
  hipError_t e;
  if (device >= 0) {
    if ((e = hipSetDevice(device)) != hipSuccess) return fail(std::string("hipSetDevice: ") + hipGetErrorString(e));
    h->device = device;
  } else {
    (void)hipGetDevice(&h->device);
  }
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0)
      h->list_grid = (uint32_t)(4 * cus);
  }
  // dynamic-LDS limits are kept per (function, device): raise them for THIS device, and say so when that fails
  if ((e = set_kernel_attributes_k2()) != hipSuccess || (e = set_kernel_attributes_k6()) != hipSuccess ||
      (e = set_kernel_attributes_k7a()) != hipSuccess || (e = set_kernel_attributes_k7r()) != hipSuccess)
    return fail(std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e));
  if ((e = cluster_limits(h->device, &h->cluster_limits)) != hipSuccess)
    return fail(std::string("cluster_limits: ") + hipGetErrorString(e));
  for (const Buffer& b : handle_buffers(h))
    if (b.bytes && (e = hipMalloc(b.ptr, b.bytes)) != hipSuccess) return fail(std::string("hipMalloc: ") + hipGetErrorString(e));
  warn_hw_queues_once();
  for (hipStream_t& s : h->stream)
    if ((e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess)
      return fail(std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e));
  if ((e = hipEventCreateWithFlags(&h->entry_done, hipEventDisableTiming)) != hipSuccess)
    return fail(std::string("hipEventCreateWithFlags: ") + hipGetErrorString(e));
  if (alloc_slot(h, h->slots[0]) != ILCC_OK) return fail(h->err);   // further slots on first asynchronous use
  if (upload_tables(h) != ILCC_OK) return fail(h->err);
  return h;
}

void ilcc_destroy(ilcc_handle* h) {
  if (!h) return;
  for (hipStream_t s : h->stream)
    if (s) (void)hipStreamSynchronize(s);
  for (Slot& sl : h->slots) free_slot(h, sl);
  for (hipStream_t s : h->stream)
    if (s) (void)hipStreamDestroy(s);
  for (const Buffer& b : handle_buffers(h))
    if (*b.ptr) (void)hipFree(*b.ptr);
  if (h->tl_ref) (void)hipEventDestroy(h->tl_ref);
  if (h->entry_done) (void)hipEventDestroy(h->entry_done);
  delete h;
}

int32_t ilcc_set_params(ilcc_handle* h, const ilcc_params* p) {
  if (!h || !p) return ILCC_BAD_ARGUMENT;
  std::string why;
  if (!params_ok(*p, why)) {
    h->err = why;
    return ILCC_BAD_ARGUMENT;
  }
  if (any_batch_in_flight(h, "ilcc_set_params")) return ILCC_BAD_ARGUMENT;
  ILCC_TRY(sync_all(h));
  const ilcc_params old = h->p;
  h->p = *p;
  int32_t st = upload_tables(h);
  for (Slot& sl : h->slots)   // the common pre-pass's buffers follow the grid (no batch is in flight here)
    if (st == ILCC_OK && sl.allocated) st = size_group_prepass(h, sl);
  h->live_hist_n = h->live_hist_at = 0;   // (live workgroups per frame of another grid or bound say nothing about this one)
  if (st != ILCC_OK) {
    // the device tables may be partly overwritten: put the previous parameter set back on the device as well, and refuse
    // further work if even that fails
    const std::string why = h->err;
    h->p = old;
    if (upload_tables(h) != ILCC_OK) h->poisoned = true;
    h->err = why;
  }
  return st;
}

int32_t ilcc_reserve(ilcc_handle* h, uint32_t labelled_points_per_frame, uint32_t roi_points_per_frame) {
  if (!h || any_batch_in_flight(h, "ilcc_reserve")) return ILCC_BAD_ARGUMENT;
  // occupied cells: a cell of side 0.57 tol holds ~4.5 points of a VLP-16 ROI and ~8 of a 64-ring one; a quarter of the
  // points is a safe capacity (a frame above it takes the slower point-level path once and the handle grows)
  raise_capacities(h, grid_lds_capacity(labelled_points_per_frame), cluster_lds_capacity(roi_points_per_frame, (uint32_t)kClusterLdsPointsMin),
                   cluster_cells_capacity(roi_points_per_frame / 4u));
  return ILCC_OK;
}

int32_t ilcc_set_result_mode(ilcc_handle* h, int32_t mode) {
  if (!h || (mode != ILCC_RESULTS_FULL && mode != ILCC_RESULTS_COMPACT) || any_batch_in_flight(h, "ilcc_set_result_mode")) return ILCC_BAD_ARGUMENT;
  h->result_mode = mode;
  return ILCC_OK;
}

// ---- The batch entries: the argument check, then run_batch

int32_t ilcc_submit_batch_device(ilcc_handle* h, const float* d_xyzi, const uint64_t* offsets, uint32_t n_frames,
                                 const float* d_clicks, int32_t* ticket) {
  if (!h || !d_xyzi || !d_clicks || !ticket) return ILCC_BAD_ARGUMENT;
  return run_batch(h, kRoiPipeline, /*on_device=*/true, d_xyzi, offsets, n_frames, d_clicks, ticket, nullptr);
}

int32_t ilcc_submit_batch(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames, const float* clicks,
                          int32_t* ticket) {
  if (!h || !xyzi || !clicks || !ticket) return ILCC_BAD_ARGUMENT;
  return run_batch(h, kRoiPipeline, /*on_device=*/false, xyzi, offsets, n_frames, clicks, ticket, nullptr);
}

int32_t ilcc_extract_batch_device(ilcc_handle* h, const float* d_xyzi, const uint64_t* offsets,
                                  uint32_t n_frames, const float* d_clicks, ilcc_result* out) {
  if (!h || !d_xyzi || !d_clicks || !out) return ILCC_BAD_ARGUMENT;
  return run_batch(h, kRoiPipeline, /*on_device=*/true, d_xyzi, offsets, n_frames, d_clicks, nullptr, out);
}

int32_t ilcc_extract_batch(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames,
                           const float* clicks, ilcc_result* out) {
  if (!h || !xyzi || !clicks || !out) return ILCC_BAD_ARGUMENT;
  return run_batch(h, kRoiPipeline, /*on_device=*/false, xyzi, offsets, n_frames, clicks, nullptr, out);
}

int32_t ilcc_extract(ilcc_handle* h, const float* xyzi, uint32_t n, const float click[3], ilcc_result* out) {
  const uint64_t off[2] = {0, n};
  return ilcc_extract_batch(h, xyzi, off, 1, click, out);
}

int32_t ilcc_chessboard_by_point_batch(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames,
                                       const float* points, int32_t min_plane_points, ilcc_result* out) {
  if (!h || !xyzi || !points || !out) return ILCC_BAD_ARGUMENT;
  ILCC_TRY(run_batch(h, kByPoint, /*on_device=*/false, xyzi, offsets, n_frames, points, nullptr, out));
  finish_chessboard_by_point(h, h->slots[0], n_frames, min_plane_points, out);
  return ILCC_OK;
}

// The same call in two halves, like ilcc_submit_batch / ilcc_wait: up to four calls in flight per handle, each whole on one of
// the handle's three streams in turn, the H2D copy of one overlapping the kernels of the others (the two tiers need no host
// decision in between: the second tier's kernels skip the frames the first has answered).  A tracker that hands over one scan at
// a time gains nothing; a recorded sequence does.
int32_t ilcc_submit_chessboard_by_point(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames,
                                        const float* points, int32_t* ticket) {
  if (!h || !xyzi || !points || !ticket) return ILCC_BAD_ARGUMENT;
  return run_batch(h, kByPoint, /*on_device=*/false, xyzi, offsets, n_frames, points, ticket, nullptr);
}

// ---- The waits: ticket_slot, then finish

int32_t ilcc_wait(ilcc_handle* h, int32_t ticket, ilcc_result* out) {
  Slot* sl = ticket_slot(h, ticket, "ilcc_wait", kRoiPipeline, out != nullptr);
  return sl ? finish(h, *sl, out) : ILCC_BAD_ARGUMENT;
}

int32_t ilcc_wait_records_device(ilcc_handle* h, int32_t ticket, ilcc_result* out, void* d_records, uint32_t n_corners,
                                 uint32_t tag_base) {
  // (out may be NULL: device records only)
  Slot* sl = ticket_slot(h, ticket, "ilcc_wait_records_device", kRoiPipeline, d_records && n_corners <= ILCC_MAX_CORNERS);
  return sl ? finish(h, *sl, out, nullptr, static_cast<float*>(d_records), n_corners, tag_base) : ILCC_BAD_ARGUMENT;
}

uint32_t ilcc_record_floats(const ilcc_handle* h, int32_t ticket) {
  const Slot* sl = busy_slot(h, ticket);
  return sl ? (uint32_t)record_floats(*sl) : 0u;
}

int32_t ilcc_wait_compact(ilcc_handle* h, int32_t ticket, float* records, uint64_t capacity_floats) {
  Slot* sl = ticket_slot(h, ticket, "ilcc_wait_compact", kRoiPipeline, records != nullptr);
  if (!sl) return ILCC_BAD_ARGUMENT;
  const uint64_t need = (uint64_t)sl->n_frames * record_floats(*sl);   // the record width was fixed when the batch was submitted
  if (capacity_floats < need) {
    h->err = "ilcc_wait_compact: the batch's records need " + std::to_string(need) + " floats, the buffer holds " +
             std::to_string(capacity_floats) + " (the batch stays in flight)";
    return ILCC_BAD_ARGUMENT;
  }
  return finish(h, *sl, nullptr, records);
}

int32_t ilcc_wait_chessboard_by_point(ilcc_handle* h, int32_t ticket, int32_t min_plane_points, ilcc_result* out) {
  Slot* sl = ticket_slot(h, ticket, "ilcc_wait_chessboard_by_point", kByPoint, out != nullptr);
  if (!sl) return ILCC_BAD_ARGUMENT;
  ILCC_TRY(finish(h, *sl, out));
  finish_chessboard_by_point(h, *sl, sl->n_frames, min_plane_points, out);
  return ILCC_OK;
}

// ---- The fetch entries: the last completed batch's records and stage buffers

int32_t ilcc_fetch_results(ilcc_handle* h, uint32_t first, uint32_t n, ilcc_result* out) {
  Slot* slp = nullptr;
  ILCC_TRY(out ? fetch_slot(h, first, n, slp) : ILCC_BAD_ARGUMENT);
  Slot& sl = *slp;
  ILCC_TRY(ensure_full(h, sl));
  const size_t row = trimmed_bytes(sl.rec_corners);
  for (uint32_t f = 0; f < n; ++f) std::memcpy(&out[f], &sl.h_res[first + f], row);
  return ILCC_OK;
}

int64_t ilcc_fetch_classes(ilcc_handle* h, uint32_t frame, uint8_t* out_class, uint64_t cap_points) {
  Slot* slp = nullptr;
  const int32_t st = fetch_slot(h, frame, 1, slp);
  if (st != ILCC_OK) return -(int64_t)st;
  Slot& sl = *slp;
  if (ensure_full(h, sl) != ILCC_OK) return -(int64_t)ILCC_HIP_ERROR;
  const ilcc_result& r = sl.h_res[frame];
  const int64_t n = (r.status == ILCC_OK || r.status == ILCC_AMBIGUOUS || r.status == ILCC_BOARD_NOT_FOUND) ? r.n_plane : 0;
  const int64_t m = std::min<int64_t>(n, (int64_t)cap_points);
  if (m > 0 && out_class &&
      hipMemcpy(out_class, sl.d_cls + sl.off[frame], (size_t)m, hipMemcpyDeviceToHost) != hipSuccess)
    return -(int64_t)ILCC_HIP_ERROR;
  return n;
}

int64_t ilcc_fetch_cloud(ilcc_handle* h, uint32_t frame, int32_t which, float* out_xyzi, uint64_t cap_points) {
  Slot* slp = nullptr;
  const int32_t st = fetch_slot(h, frame, 1, slp);
  if (st != ILCC_OK) return -(int64_t)st;
  Slot& sl = *slp;
  if (ensure_full(h, sl) != ILCC_OK) return -(int64_t)ILCC_HIP_ERROR;
  const ilcc_result& r = sl.h_res[frame];
  const float4* src = nullptr;
  int64_t n = 0;
  switch (which) {
    case ILCC_CLOUD_ROI: src = sl.d_roi; n = r.n_roi; break;
    case ILCC_CLOUD_CLUSTER: src = sl.d_cluster; n = r.n_cluster; break;
    case ILCC_CLOUD_CHESSBOARD: src = sl.d_board; n = r.n_plane; break;   // also after ILCC_BOARD_NOT_FOUND
    case ILCC_CLOUD_PCA:
      src = sl.d_pca;
      n = (r.status == ILCC_OK || r.status == ILCC_AMBIGUOUS || r.status == ILCC_DEGENERATE_HIST || r.status == ILCC_BOARD_NOT_FOUND) ? r.n_plane : 0;
      break;
    case ILCC_CLOUD_OPTIM: src = sl.d_optim; n = (r.status == ILCC_OK || r.status == ILCC_AMBIGUOUS) ? r.n_plane : 0; break;
    default: return -(int64_t)ILCC_BAD_ARGUMENT;
  }
  const int64_t m = std::min<int64_t>(n, (int64_t)cap_points);
  if (m > 0 && out_xyzi &&
      hipMemcpy(out_xyzi, src + sl.off[frame], sizeof(float4) * (size_t)m, hipMemcpyDeviceToHost) != hipSuccess)
    return -(int64_t)ILCC_HIP_ERROR;
  return n;
}

int64_t ilcc_fetch_labelled(ilcc_handle* h, uint32_t frame, float* out_yz, uint8_t* out_label, uint64_t cap_points) {
  Slot* slp = nullptr;
  const int32_t st = fetch_slot(h, frame, 1, slp);
  if (st != ILCC_OK) return -(int64_t)st;
  Slot& sl = *slp;
  uint32_t n = 0;
  if (hipMemcpy(&n, sl.d_nlab + frame, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -(int64_t)ILCC_HIP_ERROR;
  return fetch_labelled_points(sl.d_yz + sl.off[frame], sl.d_lab + sl.off[frame], n, out_yz, out_label, cap_points);
}

int64_t ilcc_fetch_walk(ilcc_handle* h, uint32_t frame, float* out_yz, uint8_t* out_label, uint64_t cap_points, uint32_t counts[2]) {
  Slot* slp = nullptr;
  const int32_t st = fetch_slot(h, frame, 1, slp);
  if (st != ILCC_OK) return -(int64_t)st;
  Slot& sl = *slp;
  if (!sl.grid) return -(int64_t)ILCC_BAD_ARGUMENT;
  uint32_t n = 0;
  if (hipMemcpy(&n, sl.d_nlab + frame, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -(int64_t)ILCC_HIP_ERROR;
  if (n > (uint32_t)kGridLdsPointsMax) n = 0;   // such a frame is walked through global memory: no layout
  if (counts) {
    if (hipMemcpy(&counts[0], sl.d_walk_mi + frame, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&counts[1], sl.d_walk_nrim + frame, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
      return -(int64_t)ILCC_HIP_ERROR;
  }
  return fetch_labelled_points(sl.d_walk_yz + sl.off[frame], sl.d_walk_lab + sl.off[frame], n, out_yz, out_label, cap_points);
}

int32_t ilcc_grid_cost(ilcc_handle* h, const float* yz, const uint8_t* label, uint32_t m, int32_t use_oob,
                       float* cost_out, int32_t* best_index, float* best_cost) {
  if (!h) return ILCC_BAD_ARGUMENT;
  const hipStream_t s = h->stream[take_stream(h)];
  ILCC_TRY(stage_labelled(h, s, yz, label, m));
  Slot& sl = h->slots[0];
  const size_t vol = (size_t)h->p.n_th * h->p.n_ty * h->p.n_tz * 2;
  float* d_vol = nullptr;
  if (cost_out) HIP_TRY(h, hipMalloc((void**)&d_vol, sizeof(float) * vol));
  struct VolGuard {   // every exit path below frees the volume
    float* p;
    ~VolGuard() { if (p) (void)hipFree(p); }
  } guard{d_vol};
  const Ctx c = diagnostic_ctx(h, sl, m);
  const uint32_t inf_bits = 0x7f800000u;
  HIP_TRY(h, hipMemcpyAsync(sl.d_bound, &inf_bits, sizeof(inf_bits), hipMemcpyHostToDevice, s));
  launch_walk_order(c, s);
  // full evaluation when the volume is wanted, the pipeline's branch-and-bound variant otherwise
  launch_grid_cost(c, whole_grid_pass(c, c.grid, c.partial), s, use_oob, d_vol, /*prune=*/d_vol == nullptr && h->p.grid_prune != 0);
  std::vector<GridPartial> part(c.grid_blocks);
  hipError_t e = hipGetLastError();   // a launch that asked for more LDS than the device grants fails HERE, not at the copy
  if (e == hipSuccess) e = hipMemcpyAsync(part.data(), sl.d_partial, sizeof(GridPartial) * c.grid_blocks, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && cost_out) e = hipMemcpyAsync(cost_out, d_vol, sizeof(float) * vol, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipEventRecord(h->entry_done, s);
  if (e == hipSuccess) e = hipEventSynchronize(h->entry_done);
  if (e != hipSuccess) {
    h->err = std::string("ilcc_grid_cost: ") + hipGetErrorString(e);
    return ILCC_HIP_ERROR;
  }
  GridPartial b = part[0];
  for (uint32_t k = 1; k < c.grid_blocks; ++k) {
    const GridPartial& t = part[k];
    if (t.cost < b.cost || (t.cost == b.cost && (t.d2 < b.d2 || (t.d2 == b.d2 && t.flat < b.flat)))) b = t;
  }
  if (best_index) *best_index = (int32_t)b.flat;
  if (best_cost) *best_cost = b.cost;
  return ILCC_OK;
}

int32_t ilcc_grid_solve(ilcc_handle* h, const float* yz, const uint8_t* label, uint32_t m, int32_t* grid_index, float* grid_cost,
                        int32_t lat[3], int32_t* phase, int64_t* cost_q, int64_t* alt_cost_q, int32_t* rounds, int32_t* hops,
                        int32_t* flags, int32_t* ties) {
  if (!h || h->p.solver != ILCC_SOLVER_GRID) {
    if (h) h->err = "ilcc_grid_solve needs ILCC_SOLVER_GRID";
    return ILCC_BAD_ARGUMENT;
  }
  const hipStream_t s = h->stream[take_stream(h)];
  ILCC_TRY(stage_labelled(h, s, yz, label, m));
  Slot& sl = h->slots[0];
  const Ctx c = diagnostic_ctx(h, sl, m);
  // what K1 resets per frame and per batch
  const uint32_t inf_bits = 0x7f800000u, zero = 0u;
  HIP_TRY(h, hipMemcpyAsync(sl.d_bound, &inf_bits, sizeof(inf_bits), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_bound_sub, &inf_bits, sizeof(inf_bits), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_tie_count, &zero, sizeof(zero), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemsetAsync(sl.d_iters, 0, sizeof(unsigned long long) * kBatchWords, s));
  ILCC_TRY(enqueue_grid_search(h, sl, c, s, 1, /*chain=*/false));
  launch_pattern_refine(c, s);
  launch_corners(c, s, 1);
  HIP_TRY(h, hipGetLastError());
  SolveRec rec{};
  ilcc_result r;
  HIP_TRY(h, hipMemcpyAsync(&rec, sl.d_solverec, sizeof(rec), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipMemcpyAsync(&r, sl.d_res, offsetof(ilcc_result, corners), hipMemcpyDeviceToHost, s));
  ILCC_TRY(sync_own(h, s));
  if (!rec.valid) {
    h->err = "ilcc_grid_solve: the grid search produced no candidate";
    return ILCC_TOO_FEW_POINTS;
  }
  const double div = (double)(h->p.refine_div > 0 ? h->p.refine_div : 1);
  if (grid_index) *grid_index = r.grid_index;
  if (grid_cost) *grid_cost = r.grid_cost;
  if (lat) {
    lat[0] = (int32_t)std::lround((rec.x[0] - h->p.th_min) / (h->p.th_step / div));
    lat[1] = (int32_t)std::lround((rec.x[1] - h->p.ty_min) / (h->p.ty_step / div));
    lat[2] = (int32_t)std::lround((rec.x[2] - h->p.tz_min) / (h->p.tz_step / div));
  }
  if (phase) *phase = rec.phase;
  if (cost_q) *cost_q = rec.cost_q;   // (not rec.sel x 2^40: a sum of 2^53 or more does not survive the double)
  if (alt_cost_q) *alt_cost_q = rec.alt_q;
  if (rounds) *rounds = rec.iters_a;
  if (hops) *hops = rec.iters_b;
  if (flags) *flags = rec.flags;
  if (ties) *ties = rec.ties;
  return ILCC_OK;
}

int32_t ilcc_get_theta_t(ilcc_handle* h, const float* yz, const uint8_t* label, uint32_t m, int32_t topleft_white,
                         int32_t use_oob, double theta_t[3], double* cost, int32_t* iterations) {
  if (!h || !theta_t) return ILCC_BAD_ARGUMENT;
  const hipStream_t s = h->stream[take_stream(h)];
  ILCC_TRY(stage_labelled(h, s, yz, label, m));
  Slot& sl = h->slots[0];
  HIP_TRY(h, hipMemcpyAsync(h->d_solve, theta_t, sizeof(double) * 3, hipMemcpyHostToDevice, s));
  const Ctx c = diagnostic_ctx(h, sl, 0);
  launch_local_solve(c, s, topleft_white, use_oob, h->d_solve, h->d_solve + 3);
  HIP_TRY(h, hipGetLastError());
  double back[5];
  HIP_TRY(h, hipMemcpyAsync(back, h->d_solve, sizeof(back), hipMemcpyDeviceToHost, s));
  ILCC_TRY(sync_own(h, s));
  theta_t[0] = back[0];
  theta_t[1] = back[1];
  theta_t[2] = back[2];
  if (cost) *cost = back[3];
  if (iterations) *iterations = (int32_t)back[4];
  return ILCC_OK;
}

int32_t ilcc_debug_reference_solve(ilcc_handle* h, const float* yz, const uint8_t* label, const uint64_t* offsets,
                                   const int32_t* status_in, uint32_t n_frames, double* rec_f64, int32_t* rec_i32,
                                   ilcc_result* results, uint32_t* lds_points) {
  if (!h || !status_in || !rec_f64 || !rec_i32 || !results) return ILCC_BAD_ARGUMENT;
  Slot& sl = h->slots[0];
  if (sl.busy) {
    h->err = "diagnostic entry while ticket 0 is in flight";
    return ILCC_BAD_ARGUMENT;
  }
  if (h->p.solver != ILCC_SOLVER_REFERENCE_LOCAL) {
    h->err = "ilcc_debug_reference_solve needs ILCC_SOLVER_REFERENCE_LOCAL";
    return ILCC_BAD_ARGUMENT;
  }
  ILCC_TRY(check_offsets(h, offsets, n_frames));
  const uint64_t total = offsets[n_frames];
  if (total > 0 && (!yz || !label)) return ILCC_BAD_ARGUMENT;
  HIP_TRY(h, hipSetDevice(h->device));
  const hipStream_t s = h->stream[take_stream(h)];
  // what K4/K5 leave behind for the back end: offsets, labelled counts (+ walk strides), and a record per frame -- zeroed but for
  // the caller's status
  std::vector<uint32_t> n_lab(n_frames), stride(n_frames);
  std::vector<ilcc_result> res(n_frames);
  std::memset(res.data(), 0, sizeof(ilcc_result) * n_frames);
  for (uint32_t f = 0; f < n_frames; ++f) {
    n_lab[f] = (uint32_t)(offsets[f + 1] - offsets[f]);
    stride[f] = walk_stride(n_lab[f]);
    res[f].status = status_in[f];
  }
  HIP_TRY(h, hipMemcpyAsync(sl.d_off, offsets, sizeof(uint64_t) * (n_frames + 1), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_res, res.data(), sizeof(ilcc_result) * n_frames, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_nlab, n_lab.data(), sizeof(uint32_t) * n_frames, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_walk, stride.data(), sizeof(uint32_t) * n_frames, hipMemcpyHostToDevice, s));
  if (total > 0) {
    HIP_TRY(h, hipMemcpyAsync(sl.d_yz, yz, sizeof(float2) * total, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(sl.d_lab, label, total, hipMemcpyHostToDevice, s));
  }
  // (a record slot the launch does not write comes back with every bit set: valid == -1, never 0 or 1)
  HIP_TRY(h, hipMemsetAsync(sl.d_solverec, 0xFF, sizeof(SolveRec) * 2 * n_frames, s));
  sl.n_frames = 0;   // the stage buffers no longer describe a batch
  // the handle's capacities as they are (diagnostic_ctx would grow the staging to the frame): the caller decides which frames
  // stay in global memory
  const Ctx c = make_ctx(h, sl, nullptr, nullptr, n_frames, 1);
  launch_reference_solve(c, s);
  launch_corners(c, s, solve_slots(c.p));
  HIP_TRY(h, hipGetLastError());
  std::vector<SolveRec> rec(2 * (size_t)n_frames);
  HIP_TRY(h, hipMemcpyAsync(rec.data(), sl.d_solverec, sizeof(SolveRec) * rec.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipMemcpyAsync(results, sl.d_res, sizeof(ilcc_result) * n_frames, hipMemcpyDeviceToHost, s));
  ILCC_TRY(sync_own(h, s));
  for (size_t k = 0; k < rec.size(); ++k) {
    const SolveRec& r = rec[k];
    const double d[ILCC_SOLVE_REC_DOUBLES] = {r.x[0], r.x[1], r.x[2], r.cost_a, r.cost_b, r.sel};
    const int32_t i[ILCC_SOLVE_REC_INTS] = {r.iters_a, r.iters_b, r.phase, r.valid};
    std::memcpy(rec_f64 + ILCC_SOLVE_REC_DOUBLES * k, d, sizeof(d));
    std::memcpy(rec_i32 + ILCC_SOLVE_REC_INTS * k, i, sizeof(i));
  }
  if (lds_points) *lds_points = c.grid_lds_points;
  return ILCC_OK;
}

int32_t ilcc_debug_locate(ilcc_handle* h, const float* yz, const uint8_t* label, const uint64_t* offsets, uint32_t n_frames,
                          uint32_t* records_out, uint32_t* bound_out) {
  if (!h || !records_out || !bound_out) return ILCC_BAD_ARGUMENT;
  Slot& sl = h->slots[0];
  if (sl.busy) {
    h->err = "diagnostic entry while ticket 0 is in flight";
    return ILCC_BAD_ARGUMENT;
  }
  if (h->p.solver != ILCC_SOLVER_GRID) {
    h->err = "ilcc_debug_locate needs ILCC_SOLVER_GRID";
    return ILCC_BAD_ARGUMENT;
  }
  ILCC_TRY(check_offsets(h, offsets, n_frames));
  const uint64_t total = offsets[n_frames];
  if (total > 0 && (!yz || !label)) return ILCC_BAD_ARGUMENT;
  HIP_TRY(h, hipSetDevice(h->device));
  // the handle's capacities as they are (see ilcc_debug_reference_solve): the caller decides which frames the anchor stages
  const Ctx c = make_ctx(h, sl, nullptr, nullptr, n_frames, 1);
  const LocatePlan lp = locate_plan(h, sl, c);
  if (locate_form(h, lp, (uint32_t)kLocateMinFrames) != kLocateFused) {
    h->err = "ilcc_debug_locate: this grid (or LDS capacity) does not take k6_locate";
    return ILCC_CAPACITY;
  }
  const hipStream_t s = h->stream[take_stream(h)];
  // what K4/K5 leave behind for the grid search and what K1 resets: offsets, labelled counts (+ walk strides), an OK record and an
  // infinite bound per frame, the batch's counters
  std::vector<uint32_t> n_lab(n_frames), stride(n_frames), bound(n_frames, 0x7f800000u);
  std::vector<ilcc_result> res(n_frames);
  std::memset(res.data(), 0, sizeof(ilcc_result) * n_frames);
  for (uint32_t f = 0; f < n_frames; ++f) {
    n_lab[f] = (uint32_t)(offsets[f + 1] - offsets[f]);
    stride[f] = walk_stride(n_lab[f]);
    res[f].status = ILCC_OK;
  }
  HIP_TRY(h, hipMemcpyAsync(sl.d_off, offsets, sizeof(uint64_t) * (n_frames + 1), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_res, res.data(), sizeof(ilcc_result) * n_frames, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_nlab, n_lab.data(), sizeof(uint32_t) * n_frames, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_walk, stride.data(), sizeof(uint32_t) * n_frames, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_bound, bound.data(), sizeof(uint32_t) * n_frames, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemsetAsync(sl.d_iters, 0, sizeof(unsigned long long) * kBatchWords, s));
  if (total > 0) {
    HIP_TRY(h, hipMemcpyAsync(sl.d_yz, yz, sizeof(float2) * total, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(sl.d_lab, label, total, hipMemcpyHostToDevice, s));
  }
  // (a record the launch does not write comes back with every bit set)
  HIP_TRY(h, hipMemsetAsync(lp.out, 0xFF, sizeof(GridPartial) * n_frames, s));
  sl.n_frames = 0;   // the stage buffers no longer describe a batch
  launch_walk_order(c, s);
  launch_locate(c, s, lp);
  HIP_TRY(h, hipGetLastError());
  static_assert(sizeof(GridPartial) == 4 * sizeof(uint32_t), "records_out: four words per frame");
  HIP_TRY(h, hipMemcpyAsync(records_out, lp.out, sizeof(GridPartial) * n_frames, hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipMemcpyAsync(bound_out, sl.d_bound, sizeof(uint32_t) * n_frames, hipMemcpyDeviceToHost, s));
  ILCC_TRY(sync_own(h, s));
  return ILCC_OK;
}

int32_t ilcc_debug_grid_solve_batch(ilcc_handle* h, const float* yz, const uint8_t* label, const uint64_t* offsets,
                                    const int32_t* status_in, uint32_t n_frames, double* rec_f64, int64_t* rec_i64, int32_t* rec_i32,
                                    ilcc_result* results, uint32_t* info) {
  if (!h) return ILCC_BAD_ARGUMENT;
  if (!status_in || !rec_f64 || !rec_i64 || !rec_i32 || !results) {
    h->err = "ilcc_debug_grid_solve_batch: null status_in or output";
    return ILCC_BAD_ARGUMENT;
  }
  Slot& sl = h->slots[0];
  if (sl.busy) {
    h->err = "diagnostic entry while ticket 0 is in flight";
    return ILCC_BAD_ARGUMENT;
  }
  if (h->p.solver != ILCC_SOLVER_GRID) {
    h->err = "ilcc_debug_grid_solve_batch needs ILCC_SOLVER_GRID";
    return ILCC_BAD_ARGUMENT;
  }
  ILCC_TRY(check_offsets(h, offsets, n_frames));
  const uint64_t total = offsets[n_frames];
  if (total > 0 && (!yz || !label)) {
    h->err = "ilcc_debug_grid_solve_batch: null points";
    return ILCC_BAD_ARGUMENT;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  const hipStream_t s = h->stream[take_stream(h)];
  // what K4/K5 leave behind for the back end -- offsets, labelled counts (+ walk strides) -- and what K1 resets: a record per frame
  // (zeroed but for the caller's status), an infinite bound and sub-bound and no near ties per frame, the batch's counters
  std::vector<uint32_t> n_lab(n_frames), stride(n_frames), bound(n_frames, 0x7f800000u);
  std::vector<ilcc_result> res(n_frames);
  std::memset(res.data(), 0, sizeof(ilcc_result) * n_frames);
  for (uint32_t f = 0; f < n_frames; ++f) {
    n_lab[f] = (uint32_t)(offsets[f + 1] - offsets[f]);
    stride[f] = walk_stride(n_lab[f]);
    res[f].status = status_in[f];
  }
  HIP_TRY(h, hipMemcpyAsync(sl.d_off, offsets, sizeof(uint64_t) * (n_frames + 1), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_res, res.data(), sizeof(ilcc_result) * n_frames, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_nlab, n_lab.data(), sizeof(uint32_t) * n_frames, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_walk, stride.data(), sizeof(uint32_t) * n_frames, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_bound, bound.data(), sizeof(uint32_t) * n_frames, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(sl.d_bound_sub, bound.data(), sizeof(uint32_t) * n_frames, hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemsetAsync(sl.d_tie_count, 0, sizeof(uint32_t) * n_frames, s));
  HIP_TRY(h, hipMemsetAsync(sl.d_iters, 0, sizeof(unsigned long long) * kBatchWords, s));
  if (total > 0) {
    HIP_TRY(h, hipMemcpyAsync(sl.d_yz, yz, sizeof(float2) * total, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(sl.d_lab, label, total, hipMemcpyHostToDevice, s));
  }
  // (a record slot no launch writes comes back with every bit set: valid == -1, never 0 or 1)
  HIP_TRY(h, hipMemsetAsync(sl.d_solverec, 0xFF, sizeof(SolveRec) * 2 * n_frames, s));
  sl.n_frames = 0;   // the stage buffers no longer describe a batch
  // the handle's capacities as they are (diagnostic_ctx would grow the staging to the frame): the caller decides which frames stay
  // in global memory.  From here on the frame count alone selects what runs, as in enqueue_impl
  const Ctx c = make_ctx(h, sl, nullptr, nullptr, n_frames, 1);
  ILCC_TRY(enqueue_grid_search(h, sl, c, s, n_frames, /*chain=*/false));
  launch_pattern_refine(c, s);
  launch_corners(c, s, 1);
  HIP_TRY(h, hipGetLastError());
  std::vector<SolveRec> rec(2 * (size_t)n_frames);
  std::vector<ilcc_result> back(n_frames);
  HIP_TRY(h, hipMemcpyAsync(rec.data(), sl.d_solverec, sizeof(SolveRec) * rec.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipMemcpyAsync(back.data(), sl.d_res, sizeof(ilcc_result) * n_frames, hipMemcpyDeviceToHost, s));
  ILCC_TRY(sync_own(h, s));
  for (uint32_t f = 0; f < n_frames; ++f) {
    const SolveRec& r = rec[2 * (size_t)f];
    const double d[ILCC_GRID_REC_DOUBLES] = {r.x[0], r.x[1], r.x[2]};
    const int64_t q[ILCC_GRID_REC_INT64S] = {(int64_t)r.cost_q, (int64_t)r.alt_q};   // (not r.sel x 2^40: see ilcc_grid_solve)
    const int32_t i[ILCC_GRID_REC_INTS] = {r.iters_a, r.iters_b, r.phase, r.valid, r.flags, r.ties};
    std::memcpy(rec_f64 + ILCC_GRID_REC_DOUBLES * (size_t)f, d, sizeof(d));
    std::memcpy(rec_i64 + ILCC_GRID_REC_INT64S * (size_t)f, q, sizeof(q));
    std::memcpy(rec_i32 + ILCC_GRID_REC_INTS * (size_t)f, i, sizeof(i));
    std::memcpy(&results[f], &back[f], offsetof(ilcc_result, corners));
  }
  if (info) {
    info[0] = c.grid_lds_points;
    info[1] = (uint32_t)locate_form(h, locate_plan(h, sl, c), n_frames);
    info[2] = h->full_pass_last[0];
    info[3] = (uint32_t)(n_frames <= (uint32_t)kSmallBatchFrames ? kRefineThreadsSmallBatch : kRefineThreads);
  }
  return ILCC_OK;
}

int32_t ilcc_pattern_refine(ilcc_handle* h, const float* yz, const uint8_t* label, uint32_t m, int32_t lat[3],
                            int32_t* phase, int64_t* cost_q, int64_t* alt_cost_q, int32_t* rounds, int32_t* hops) {
  if (!h || !lat || !phase) return ILCC_BAD_ARGUMENT;
  if (lat[0] < h->th_lat_lo || lat[0] > h->th_lat_hi || (*phase != 0 && *phase != 1)) {
    // the kernel indexes its cos/sin table with lat[0] (the basin check reads it unguarded)
    h->err = "ilcc_pattern_refine: theta lattice coordinate outside [th_min - refine_th_margin, th_max + refine_th_margin] steps";
    return ILCC_BAD_ARGUMENT;
  }
  const hipStream_t s = h->stream[take_stream(h)];
  ILCC_TRY(stage_labelled(h, s, yz, label, m));
  Slot& sl = h->slots[0];
  RefineOut io{};
  io.lat[0] = lat[0];
  io.lat[1] = lat[1];
  io.lat[2] = lat[2];
  io.phase = *phase;
  HIP_TRY(h, hipMemcpyAsync(h->d_refine_io, &io, sizeof(io), hipMemcpyHostToDevice, s));
  const Ctx c = diagnostic_ctx(h, sl, 0);
  launch_pattern_refine_test(c, s, h->d_refine_io);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(&io, h->d_refine_io, sizeof(io), hipMemcpyDeviceToHost, s));
  ILCC_TRY(sync_own(h, s));
  lat[0] = io.lat[0];
  lat[1] = io.lat[1];
  lat[2] = io.lat[2];
  *phase = io.phase;
  if (cost_q) *cost_q = io.cost_q;
  if (alt_cost_q) *alt_cost_q = io.alt_q;
  if (rounds) *rounds = io.rounds;
  if (hops) *hops = io.hops;
  return ILCC_OK;
}

int32_t ilcc_debug_timeline_enable(ilcc_handle* h, int32_t on) {
  if (!h) return ILCC_BAD_ARGUMENT;
  HIP_TRY(h, hipSetDevice(h->device));
  h->tl_rows.clear();
  h->tl_on = on != 0;
  if (h->tl_on) {
    if (!h->tl_ref) HIP_TRY(h, hipEventCreate(&h->tl_ref));
    HIP_TRY(h, hipEventRecord(h->tl_ref, h->stream[0]));
    HIP_TRY(h, hipEventSynchronize(h->tl_ref));
  }
  return ILCC_OK;
}

int32_t ilcc_debug_separate_launches(ilcc_handle* h, int32_t on) {
  if (!h || any_batch_in_flight(h, "ilcc_debug_separate_launches")) return ILCC_BAD_ARGUMENT;
  h->separate_launches = on != 0;
  return ILCC_OK;
}

int32_t ilcc_debug_full_pass_launch(ilcc_handle* h, int32_t mode, uint32_t workgroups) {
  if (!h || any_batch_in_flight(h, "ilcc_debug_full_pass_launch")) return ILCC_BAD_ARGUMENT;
  if ((mode != ILCC_FULL_PASS_RULE && mode != ILCC_FULL_PASS_GRID && mode != ILCC_FULL_PASS_LISTED) || (mode == ILCC_FULL_PASS_LISTED && workgroups == 0u)) {
    h->err = "ilcc_debug_full_pass_launch: mode must be ILCC_FULL_PASS_RULE, _GRID or _LISTED, the last with at least one workgroup";
    return ILCC_BAD_ARGUMENT;
  }
  h->full_pass_mode = mode;
  h->full_pass_forced_g = mode == ILCC_FULL_PASS_LISTED ? workgroups : 0u;
  return ILCC_OK;
}

int32_t ilcc_debug_full_pass_rule(int64_t observed_live, uint32_t n_th, uint32_t n_frames, uint32_t* workgroups) {
  uint32_t g = 0;
  const int32_t form = full_pass_rule(observed_live, n_th, n_frames, &g);
  if (workgroups) *workgroups = g;
  return form;
}

int32_t ilcc_debug_full_pass_last(const ilcc_handle* h, uint32_t out[ILCC_FULL_PASS_LAST_WORDS]) {
  if (!h || !out) return ILCC_BAD_ARGUMENT;
  for (int k = 0; k < ILCC_FULL_PASS_LAST_WORDS; ++k) out[k] = h->full_pass_last[k];
  return ILCC_OK;
}

int32_t ilcc_debug_cluster_home(ilcc_handle* h, int32_t home) {
  if (!h || any_batch_in_flight(h, "ilcc_debug_cluster_home")) return ILCC_BAD_ARGUMENT;
  if (home != ILCC_CLUSTER_HOME_RULE && home != ILCC_CLUSTER_HOME_LDS && home != ILCC_CLUSTER_HOME_L2) {
    h->err = "ilcc_debug_cluster_home: home must be ILCC_CLUSTER_HOME_RULE, _LDS or _L2";
    return ILCC_BAD_ARGUMENT;
  }
  h->cluster_home = home;
  return ILCC_OK;
}

int32_t ilcc_debug_cluster_launch(const ilcc_handle* h, uint32_t out[ILCC_CLUSTER_LAUNCH_WORDS]) {
  if (!h || !out) return ILCC_BAD_ARGUMENT;
  out[0] = (uint32_t)h->cluster_last.home;
  out[1] = h->cluster_last.lds_bytes;
  out[2] = h->cluster_last.threads;
  out[3] = h->cluster_limits.static_lds;
  out[4] = h->cluster_limits.lds_per_cu;
  out[5] = h->cluster_limits.cus;
  out[6] = h->cluster_fallback_last;
  out[7] = kFallbackGrid;
  return ILCC_OK;
}

int32_t ilcc_debug_group_prepass(ilcc_handle* h, uint32_t* states_out, uint32_t* mask_out, uint32_t dims_out[2], uint32_t* bound_out) {
  if (!h || !dims_out || any_batch_in_flight(h, "ilcc_debug_group_prepass")) return ILCC_BAD_ARGUMENT;
  HIP_TRY(h, hipSetDevice(h->device));
  const Slot& sl = h->slots[0];
  // (the conditions under which enqueue_grid_search launches k6_group_prepass for a one-frame call)
  const GroupPrepassPlan gp = group_prepass_plan(h->p);
  const bool ran = gp.on && sl.d_grp_alive && sl.d_grp_mask && gp.groups <= sl.grp_alive_cap && (size_t)gp.groups * gp.words <= sl.grp_mask_cap;
  dims_out[0] = ran ? gp.groups : 0u;
  dims_out[1] = ran ? gp.words : 0u;
  if (bound_out && sl.d_bound) HIP_TRY(h, hipMemcpy(bound_out, sl.d_bound, sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (!ran) return ILCC_OK;
  if (states_out) HIP_TRY(h, hipMemcpy(states_out, sl.d_grp_alive, sizeof(uint32_t) * gp.groups, hipMemcpyDeviceToHost));
  if (mask_out) HIP_TRY(h, hipMemcpy(mask_out, sl.d_grp_mask, sizeof(uint32_t) * gp.groups * gp.words, hipMemcpyDeviceToHost));
  return ILCC_OK;
}

int64_t ilcc_debug_solve_walk(ilcc_handle* h, float* out_yz, uint8_t* out_label, uint64_t cap_points, uint32_t counts[2]) {
  if (!h || any_batch_in_flight(h, "ilcc_debug_solve_walk")) return -(int64_t)ILCC_BAD_ARGUMENT;
  if (hipSetDevice(h->device) != hipSuccess) return -(int64_t)ILCC_HIP_ERROR;
  const Slot& sl = h->slots[0];
  if (!sl.d_nlab || !sl.d_walk_yz || !sl.d_walk_lab || !sl.d_walk_mi || !sl.d_walk_nrim) return -(int64_t)ILCC_BAD_ARGUMENT;
  uint32_t n = 0;
  if (hipMemcpy(&n, sl.d_nlab, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -(int64_t)ILCC_HIP_ERROR;
  if (n > (uint32_t)kGridLdsPointsMax || n > h->max_points) n = 0;   // such a frame is walked through global memory: no layout
  if (counts) {
    if (hipMemcpy(&counts[0], sl.d_walk_mi, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&counts[1], sl.d_walk_nrim, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
      return -(int64_t)ILCC_HIP_ERROR;
  }
  return fetch_labelled_points(sl.d_walk_yz, sl.d_walk_lab, n, out_yz, out_label, cap_points);
}

int32_t ilcc_debug_timeline_fetch(ilcc_handle* h, double* rows, uint32_t cap_rows) {
  if (!h || (!rows && cap_rows)) return -ILCC_BAD_ARGUMENT;
  const size_t have = h->tl_rows.size() / ILCC_TIMELINE_COLS;
  const size_t n = std::min<size_t>(have, cap_rows);
  if (n) std::memcpy(rows, h->tl_rows.data(), sizeof(double) * n * ILCC_TIMELINE_COLS);
  h->tl_rows.clear();
  return (int32_t)n;
}

void ilcc_get_timing(const ilcc_handle* h, ilcc_timing* t) {
  if (h && t) *t = h->timing;
}
void ilcc_reset_timing(ilcc_handle* h) {
  if (h) h->timing = ilcc_timing{};
}

}  // extern "C"
