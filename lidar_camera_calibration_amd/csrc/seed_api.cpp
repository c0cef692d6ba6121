// seed_api.cpp -- the entries of include/ilcc_seed.h: the scratch layout and host chain of K15 (k15_seed_components.hip), the
// host finishing behind it (seed_host.cpp), and ilcc_extract_auto*, which lays every proposal out as a frame of one ordinary batch.
// Every planar entry (K15p) is its ordinary sibling with a set ilcc_seed_planar_params pointer: one implementation each.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstring>
#include <vector>

#include "host_util.h"
#include "k15_seed.h"

using namespace ilcc;

namespace {

struct Layout {   // byte offsets of the parts of the scratch, each on a 256-byte boundary
  uint64_t frames, counters, tab_key, tab_ord, cell_key, parent, mom, packed, total, slots;
  uint64_t core, total_planar;   // K15p: the flag array lies behind the ordinary parts, which keep their places
};

// hash-set slots that serve any split of `points` into `frames`: a frame's set is max(64, < 4 n) slots
Layout layout(uint32_t frames, uint64_t points, uint32_t max_components) {
  Layout l{};
  l.slots = (uint64_t)ILCC_SEED_TABLE_MIN * frames + 4 * points;
  const uint64_t cells = points ? points : 1;
  uint64_t at = 0;
  auto part = [&](uint64_t bytes) {
    const uint64_t here = at;
    at += align256(bytes);
    return here;
  };
  l.frames = part(sizeof(SeedFrame) * frames);
  l.counters = part(8ull * frames);
  l.tab_key = part(4 * l.slots);
  l.tab_ord = part(4 * l.slots);
  l.cell_key = part(4 * cells);
  l.parent = part(4 * cells);
  l.mom = part(8ull * kSeedMoments * cells);
  l.packed = part(8ull * ILCC_SEED_RECORD_WORDS * max_components * frames);
  l.total = at;
  l.core = part(cells);
  l.total_planar = at;
  return l;
}

bool counts_ok(const ilcc_seed_params& sp) {
  return sp.cluster_min >= 1 && sp.max_components >= 1 && sp.max_components <= 65536 && sp.max_seeds >= 1 && sp.max_seeds <= 65536 &&
         sp.board_w >= 1 && sp.board_h >= 1 && sp.grid_length > 0;
}

using Record = std::array<int64_t, ILCC_SEED_RECORD_WORDS>;

thread_local float g_launch_ms[kSeedLaunches] = {};                // ilcc_debug_seed_launch_ms
thread_local float g_planar_launch_ms[kSeedPlanarLaunches] = {};   // ilcc_debug_seed_planar_launch_ms

struct LaunchEvents {   // HIP events in front of, between and behind K15's launches, destroyed on scope exit
  hipEvent_t ev[kSeedPlanarLaunches + 1] = {};
  ~LaunchEvents() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// K15 on a batch in HBM: per frame the sorted records (records[f]) and whether the frame overflowed max_components.
// planar: false = the ordinary components (pp is not read); true = the components of core cells under *pp
int32_t seed_components(ilcc_handle* h, const float* d_xyzi, const uint64_t* offsets, uint32_t n_frames, const ilcc_seed_params* sp,
                        bool planar, const ilcc_seed_planar_params* pp, void* d_scratch, hipStream_t s, std::vector<std::vector<Record>>* records, std::vector<uint8_t>* overflow) {
  if (!h) return ILCC_BAD_ARGUMENT;
  if (!d_xyzi || !offsets || !sp || !d_scratch || n_frames == 0 || (planar && !pp)) return handle_fail(h, ILCC_BAD_ARGUMENT, "seed: null pointer or no frames");
  if ((reinterpret_cast<uintptr_t>(d_scratch) & 255u) != 0) return handle_fail(h, ILCC_BAD_ARGUMENT, "seed: scratch must be 256-byte aligned");
  const HandleView hv = handle_view(h);
  if (n_frames > hv.max_frames || n_frames > 65535u) return handle_fail(h, ILCC_CAPACITY, "seed: n_frames exceeds the handle's max_frames (or 65535)");
  if (offsets[0] != 0) return handle_fail(h, ILCC_BAD_ARGUMENT, "offsets[0] must be 0");
  uint32_t max_n = 0;
  for (uint32_t f = 0; f < n_frames; ++f) {
    if (offsets[f + 1] < offsets[f] || offsets[f + 1] - offsets[f] > ILCC_SEED_FRAME_POINTS_MAX)
      return handle_fail(h, ILCC_BAD_ARGUMENT, "seed: offsets must be non-decreasing, frames <= 2^28 points");
    max_n = std::max(max_n, (uint32_t)(offsets[f + 1] - offsets[f]));
  }
  const uint64_t total = offsets[n_frames];
  if (total > hv.max_points) return handle_fail(h, ILCC_CAPACITY, "seed: total points exceed the handle's max_total_points");
  if (!counts_ok(*sp)) return handle_fail(h, ILCC_BAD_ARGUMENT, "seed: cluster_min, max_components, max_seeds and the board must be positive");
  SeedGrid g{};
  if (!seed_grid(*sp, hv.max_points, &g)) return handle_fail(h, ILCC_BAD_ARGUMENT, "seed: cell and range must be positive, range / cell at most 511 cells");
  double flat_q2 = 0, spread_q2 = 0, own_q2 = 0;
  if (planar) {
    if (!seed_planar_thresholds(*pp, &flat_q2, &spread_q2, &own_q2)) return handle_fail(h, ILCC_BAD_ARGUMENT, "seed: planar_rms, min_spread and own_rms must be positive");
    if (!seed_planar_frame_fits(max_n, g)) return handle_fail(h, ILCC_BAD_ARGUMENT, "seed: planar seeds need points 2 ceil(1024 cell) < 2^31 in every frame");
  }

  hipError_t e;
  if ((e = hipSetDevice(hv.device)) != hipSuccess) return handle_fail(h, ILCC_HIP_ERROR, std::string("hipSetDevice: ") + hipGetErrorString(e));
  const Layout l = layout(n_frames, total, (uint32_t)sp->max_components);
  uint8_t* base = static_cast<uint8_t*>(d_scratch);
  std::vector<SeedFrame> fr(n_frames);
  uint64_t tab = 0;
  for (uint32_t f = 0; f < n_frames; ++f) {
    const uint32_t n = (uint32_t)(offsets[f + 1] - offsets[f]);
    const uint32_t size = ilcc_seed_table_size(n);
    uint32_t bits = 0;
    while ((1u << bits) < size) ++bits;
    fr[f] = SeedFrame{offsets[f], tab, n, size - 1u, 32u - bits, 0u};
    tab += size;
  }
  SeedCtx c{};
  c.xyzi = reinterpret_cast<const float4*>(d_xyzi);
  c.fr = reinterpret_cast<const SeedFrame*>(base + l.frames);
  c.n_frames = n_frames;
  c.cluster_min = (uint32_t)sp->cluster_min;
  c.max_components = (uint32_t)sp->max_components;
  c.g = g;
  c.slots_total = tab;   // <= l.slots
  c.counters = reinterpret_cast<uint32_t*>(base + l.counters);
  c.tab_key = reinterpret_cast<uint32_t*>(base + l.tab_key);
  c.tab_ord = reinterpret_cast<uint32_t*>(base + l.tab_ord);
  c.cell_key = reinterpret_cast<uint32_t*>(base + l.cell_key);
  c.parent = reinterpret_cast<uint32_t*>(base + l.parent);
  c.mom = reinterpret_cast<long long*>(base + l.mom);
  c.packed = reinterpret_cast<long long*>(base + l.packed);
  c.core = planar ? base + l.core : nullptr;
  c.flat_q2 = flat_q2;
  c.spread_q2 = spread_q2;
  c.own_q2 = own_q2;

  std::vector<uint32_t> counters(2ull * n_frames);
  std::vector<int64_t> packed((uint64_t)ILCC_SEED_RECORD_WORDS * sp->max_components * n_frames);
  auto hip = [&](hipError_t err, const char* what) {
    return err == hipSuccess ? ILCC_OK : handle_fail(h, ILCC_HIP_ERROR, std::string(what) + ": " + hipGetErrorString(err));
  };
  int32_t st;
  if ((st = hip(hipMemcpyAsync(base + l.frames, fr.data(), sizeof(SeedFrame) * n_frames, hipMemcpyHostToDevice, s), "hipMemcpyAsync")) != ILCC_OK) return st;
  LaunchEvents le;
  const int n_launches = planar ? kSeedPlanarLaunches : kSeedLaunches;
  for (int k = 0; k <= n_launches; ++k)
    if ((st = hip(hipEventCreate(&le.ev[k]), "hipEventCreate")) != ILCC_OK) return st;
  launch_seed_components(c, max_n, s, le.ev);
  if ((st = hip(hipGetLastError(), "K15 launch")) != ILCC_OK) return st;
  if ((st = hip(hipMemcpyAsync(counters.data(), c.counters, 8ull * n_frames, hipMemcpyDeviceToHost, s), "hipMemcpyAsync")) != ILCC_OK) return st;
  if ((st = hip(hipMemcpyAsync(packed.data(), c.packed, 8ull * packed.size(), hipMemcpyDeviceToHost, s), "hipMemcpyAsync")) != ILCC_OK) return st;
  if ((st = hip(hipStreamSynchronize(s), "hipStreamSynchronize")) != ILCC_OK) return st;
  float* launch_ms = planar ? g_planar_launch_ms : g_launch_ms;
  for (int k = 0; k < n_launches; ++k)
    if (hipEventElapsedTime(&launch_ms[k], le.ev[k], le.ev[k + 1]) != hipSuccess) launch_ms[k] = 0.f;

  records->assign(n_frames, {});
  overflow->assign(n_frames, 0);
  for (uint32_t f = 0; f < n_frames; ++f) {
    const uint32_t met = counters[2 * f + 1];
    if (met > (uint32_t)sp->max_components) {
      (*overflow)[f] = 1;
      continue;
    }
    std::vector<Record>& out = (*records)[f];
    out.resize(met);
    if (met) std::memcpy(out.data(), packed.data() + (uint64_t)ILCC_SEED_RECORD_WORDS * sp->max_components * f, sizeof(Record) * met);
    std::sort(out.begin(), out.end(), [](const Record& a, const Record& b) { return a[0] < b[0]; });   // the pack's order is the threads'
  }
  return ILCC_OK;
}

// a device copy of a host batch plus K15's scratch, for the host-buffer entries
struct HostBatch {
  DeviceBuffer xyzi, scratch;
};

int32_t stage_host_batch(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames, const ilcc_seed_params* sp, bool planar,
                         const ilcc_seed_planar_params* pp, bool want_scratch, HostBatch* b) {
  if (!h) return ILCC_BAD_ARGUMENT;
  if (!xyzi || !offsets || !sp || n_frames == 0 || (planar && !pp)) return handle_fail(h, ILCC_BAD_ARGUMENT, "seed: null pointer or no frames");
  const HandleView hv = handle_view(h);
  if (n_frames > hv.max_frames || n_frames > 65535u) return handle_fail(h, ILCC_CAPACITY, "seed: n_frames exceeds the handle's max_frames (or 65535)");
  if (offsets[0] != 0) return handle_fail(h, ILCC_BAD_ARGUMENT, "offsets[0] must be 0");
  for (uint32_t f = 0; f < n_frames; ++f)
    if (offsets[f + 1] < offsets[f]) return handle_fail(h, ILCC_BAD_ARGUMENT, "seed: offsets must be non-decreasing");
  const uint64_t total = offsets[n_frames];
  if (total > hv.max_points) return handle_fail(h, ILCC_CAPACITY, "seed: total points exceed the handle's max_total_points");
  if (!counts_ok(*sp)) return handle_fail(h, ILCC_BAD_ARGUMENT, "seed: cluster_min, max_components, max_seeds and the board must be positive");
  hipError_t e;
  if ((e = hipSetDevice(hv.device)) != hipSuccess) return handle_fail(h, ILCC_HIP_ERROR, std::string("hipSetDevice: ") + hipGetErrorString(e));
  if ((e = hipMalloc(&b->xyzi.p, 16 * (total ? total : 1))) != hipSuccess) return handle_fail(h, ILCC_HIP_ERROR, std::string("hipMalloc: ") + hipGetErrorString(e));
  const Layout l = layout(n_frames, total, (uint32_t)sp->max_components);
  if (want_scratch && (e = hipMalloc(&b->scratch.p, planar ? l.total_planar : l.total)) != hipSuccess)
    return handle_fail(h, ILCC_HIP_ERROR, std::string("hipMalloc: ") + hipGetErrorString(e));
  if (total && (e = hipMemcpy(b->xyzi.p, xyzi, 16 * total, hipMemcpyHostToDevice)) != hipSuccess)
    return handle_fail(h, ILCC_HIP_ERROR, std::string("hipMemcpy: ") + hipGetErrorString(e));
  return ILCC_OK;
}

// the accept rule of ilcc_extract_auto*
bool accepted(const ilcc_result& r, const ilcc_seed_params& sp) {
  return r.status == ILCC_OK && !(r.flags & ILCC_FLAG_LOW_COVERAGE) && (double)r.n_oob <= sp.max_oob_share * (double)(r.n_black + r.n_white);
}

int32_t propose_device(ilcc_handle* h, const float* d_xyzi, const uint64_t* offsets, uint32_t n_frames, const ilcc_seed_params* sp, bool planar,
                       const ilcc_seed_planar_params* pp, void* d_scratch, ilcc_seed* out_seeds, int32_t* out_counts, void* hip_stream) {
  if (!h) return ILCC_BAD_ARGUMENT;
  if (!out_seeds || !out_counts) return handle_fail(h, ILCC_BAD_ARGUMENT, "seed: null output");
  std::vector<std::vector<Record>> records;
  std::vector<uint8_t> overflow;
  const int32_t st = seed_components(h, d_xyzi, offsets, n_frames, sp, planar, pp, d_scratch, static_cast<hipStream_t>(hip_stream), &records, &overflow);
  if (st != ILCC_OK) return st;
  for (uint32_t f = 0; f < n_frames; ++f) {
    if (overflow[f]) {
      out_counts[f] = -(int32_t)ILCC_CAPACITY;
      continue;
    }
    out_counts[f] = seed_rank(records[f].empty() ? nullptr : records[f][0].data(), (int32_t)records[f].size(), *sp, out_seeds + (uint64_t)f * sp->max_seeds);
  }
  return ILCC_OK;
}

int32_t propose_host(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames, const ilcc_seed_params* sp, bool planar,
                     const ilcc_seed_planar_params* pp, ilcc_seed* out_seeds, int32_t* out_counts) {
  if (!h) return ILCC_BAD_ARGUMENT;
  if (!out_seeds || !out_counts) return handle_fail(h, ILCC_BAD_ARGUMENT, "seed: null output");
  HostBatch b;
  const int32_t st = stage_host_batch(h, xyzi, offsets, n_frames, sp, planar, pp, true, &b);
  if (st != ILCC_OK) return st;
  return propose_device(h, static_cast<const float*>(b.xyzi.p), offsets, n_frames, sp, planar, pp, b.scratch.p, out_seeds, out_counts, nullptr);
}

int32_t debug_components(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames, const ilcc_seed_params* sp, bool planar,
                         const ilcc_seed_planar_params* pp, void* d_scratch, uint32_t frame, int64_t* out_records, uint32_t cap_records, int32_t* out_n) {
  if (!h) return ILCC_BAD_ARGUMENT;
  if (!out_records || !out_n || frame >= n_frames) return handle_fail(h, ILCC_BAD_ARGUMENT, "seed: null output or no such frame");
  HostBatch b;
  int32_t st = stage_host_batch(h, xyzi, offsets, n_frames, sp, planar, pp, d_scratch == nullptr, &b);
  if (st != ILCC_OK) return st;
  std::vector<std::vector<Record>> records;
  std::vector<uint8_t> overflow;
  st = seed_components(h, static_cast<const float*>(b.xyzi.p), offsets, n_frames, sp, planar, pp, d_scratch ? d_scratch : b.scratch.p, nullptr, &records, &overflow);
  if (st != ILCC_OK) return st;
  if (overflow[frame] || records[frame].size() > cap_records) return handle_fail(h, ILCC_CAPACITY, "seed: more components than max_components / cap_records in this frame");
  if (!records[frame].empty()) std::memcpy(out_records, records[frame].data(), sizeof(Record) * records[frame].size());
  *out_n = (int32_t)records[frame].size();
  return ILCC_OK;
}

int32_t extract_auto_batch(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames, const ilcc_seed_params* sp, bool planar,
                           const ilcc_seed_planar_params* pp, ilcc_result* out, float* out_seed, int32_t* out_rank) {
  if (!h) return ILCC_BAD_ARGUMENT;
  if (!out || !out_seed || !out_rank) return handle_fail(h, ILCC_BAD_ARGUMENT, "extract_auto: null output");
  HostBatch b;
  int32_t st = stage_host_batch(h, xyzi, offsets, n_frames, sp, planar, pp, true, &b);
  if (st != ILCC_OK) return st;
  std::vector<ilcc_seed> seeds((uint64_t)n_frames * sp->max_seeds);
  std::vector<int32_t> counts(n_frames);
  st = propose_device(h, static_cast<const float*>(b.xyzi.p), offsets, n_frames, sp, planar, pp, b.scratch.p, seeds.data(), counts.data(), nullptr);
  if (st != ILCC_OK) return st;

  // every candidate becomes a frame of one ordinary batch
  const HandleView hv = handle_view(h);
  uint64_t cand = 0, cand_points = 0;
  for (uint32_t f = 0; f < n_frames; ++f) {
    const uint64_t k = counts[f] > 0 ? (uint64_t)counts[f] : 0;
    cand += k;
    cand_points += k * (offsets[f + 1] - offsets[f]);
  }
  if (cand > hv.max_frames || cand_points > hv.max_points)
    return handle_fail(h, ILCC_CAPACITY, "extract_auto: the candidates exceed the handle's max_frames / max_total_points (size it for max_seeds times the call)");
  std::vector<ilcc_result> res(cand);
  std::memset(static_cast<void*>(res.data()), 0, sizeof(ilcc_result) * cand);
  if (cand > 0) {
    DeviceBuffer d_cand, d_clicks;
    hipError_t e;
    if ((e = hipMalloc(&d_cand.p, 16 * (cand_points ? cand_points : 1))) != hipSuccess || (e = hipMalloc(&d_clicks.p, 12 * cand)) != hipSuccess)
      return handle_fail(h, ILCC_HIP_ERROR, std::string("hipMalloc: ") + hipGetErrorString(e));
    std::vector<uint64_t> off(cand + 1, 0);
    std::vector<float> clicks(3 * cand);
    uint64_t at = 0;
    for (uint32_t f = 0; f < n_frames; ++f)
      for (int32_t k = 0; k < counts[f]; ++k) {
        const uint64_t n = offsets[f + 1] - offsets[f];
        if (n && (e = hipMemcpyAsync(static_cast<uint8_t*>(d_cand.p) + 16 * off[at], static_cast<const uint8_t*>(b.xyzi.p) + 16 * offsets[f], 16 * n,
                                     hipMemcpyDeviceToDevice, nullptr)) != hipSuccess)
          return handle_fail(h, ILCC_HIP_ERROR, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
        std::memcpy(&clicks[3 * at], seeds[(uint64_t)f * sp->max_seeds + k].centroid, 12);
        off[at + 1] = off[at] + n;
        ++at;
      }
    if ((e = hipMemcpyAsync(d_clicks.p, clicks.data(), 12 * cand, hipMemcpyHostToDevice, nullptr)) != hipSuccess || (e = hipStreamSynchronize(nullptr)) != hipSuccess)
      return handle_fail(h, ILCC_HIP_ERROR, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
    st = ilcc_extract_batch_device(h, static_cast<const float*>(d_cand.p), off.data(), (uint32_t)cand, static_cast<const float*>(d_clicks.p), res.data());
    if (st != ILCC_OK) return st;
  }

  // per cloud: the first accepted candidate in rank order.  Like ilcc_wait, a record is its head and the corners of the handle's board
  const size_t rec_bytes = offsetof(ilcc_result, corners) + 12u * (size_t)((hv.p.board_w - 1) * (hv.p.board_h - 1));
  uint64_t at = 0;
  for (uint32_t f = 0; f < n_frames; ++f) {
    const int32_t k_f = counts[f] > 0 ? counts[f] : 0;
    if (k_f == 0) {
      std::memset(static_cast<void*>(&out[f]), 0, offsetof(ilcc_result, corners));
      out[f].status = ILCC_BOARD_NOT_FOUND;
      out[f].n_points = (int32_t)(offsets[f + 1] - offsets[f]);
      out_seed[3 * f] = out_seed[3 * f + 1] = out_seed[3 * f + 2] = 0.f;
      out_rank[f] = -1;
      continue;
    }
    int32_t pick = -1;
    for (int32_t k = 0; k < k_f && pick < 0; ++k)
      if (accepted(res[at + k], *sp)) pick = k;
    const int32_t from = pick < 0 ? 0 : pick;
    std::memcpy(static_cast<void*>(&out[f]), &res[at + from], rec_bytes);
    if (pick < 0) out[f].status = ILCC_BOARD_NOT_FOUND;
    std::memcpy(&out_seed[3 * f], seeds[(uint64_t)f * sp->max_seeds + from].centroid, 12);
    out_rank[f] = pick;
    at += k_f;
  }
  return ILCC_OK;
}

}  // namespace

extern "C" {

uint64_t ilcc_seed_scratch_bytes(uint32_t n_frames, uint64_t total_points, const ilcc_seed_params* sp) {
  if (!sp || sp->max_components < 1) return 0;
  return layout(n_frames, total_points, (uint32_t)sp->max_components).total;
}

uint64_t ilcc_seed_planar_scratch_bytes(uint32_t n_frames, uint64_t total_points, const ilcc_seed_params* sp) {
  if (!sp || sp->max_components < 1) return 0;
  return layout(n_frames, total_points, (uint32_t)sp->max_components).total_planar;
}

void ilcc_debug_seed_launch_ms(float out[ILCC_SEED_LAUNCHES]) {
  for (int k = 0; k < kSeedLaunches; ++k) out[k] = g_launch_ms[k];
}

void ilcc_debug_seed_planar_launch_ms(float out[ILCC_SEED_PLANAR_LAUNCHES]) {
  for (int k = 0; k < kSeedPlanarLaunches; ++k) out[k] = g_planar_launch_ms[k];
}

int32_t ilcc_propose_seeds_device(ilcc_handle* h, const float* d_xyzi, const uint64_t* offsets, uint32_t n_frames, const ilcc_seed_params* sp,
                                  void* d_scratch, ilcc_seed* out_seeds, int32_t* out_counts, void* hip_stream) {
  return propose_device(h, d_xyzi, offsets, n_frames, sp, false, nullptr, d_scratch, out_seeds, out_counts, hip_stream);
}
int32_t ilcc_propose_seeds_planar_device(ilcc_handle* h, const float* d_xyzi, const uint64_t* offsets, uint32_t n_frames, const ilcc_seed_params* sp,
                                         const ilcc_seed_planar_params* pp, void* d_scratch, ilcc_seed* out_seeds, int32_t* out_counts, void* hip_stream) {
  return propose_device(h, d_xyzi, offsets, n_frames, sp, true, pp, d_scratch, out_seeds, out_counts, hip_stream);
}

int32_t ilcc_propose_seeds(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames, const ilcc_seed_params* sp,
                           ilcc_seed* out_seeds, int32_t* out_counts) {
  return propose_host(h, xyzi, offsets, n_frames, sp, false, nullptr, out_seeds, out_counts);
}
int32_t ilcc_propose_seeds_planar(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames, const ilcc_seed_params* sp,
                                  const ilcc_seed_planar_params* pp, ilcc_seed* out_seeds, int32_t* out_counts) {
  return propose_host(h, xyzi, offsets, n_frames, sp, true, pp, out_seeds, out_counts);
}

int32_t ilcc_debug_seed_components(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames, const ilcc_seed_params* sp,
                                   void* d_scratch, uint32_t frame, int64_t* out_records, uint32_t cap_records, int32_t* out_n) {
  return debug_components(h, xyzi, offsets, n_frames, sp, false, nullptr, d_scratch, frame, out_records, cap_records, out_n);
}
int32_t ilcc_debug_seed_planar_components(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames, const ilcc_seed_params* sp,
                                          const ilcc_seed_planar_params* pp, void* d_scratch, uint32_t frame, int64_t* out_records,
                                          uint32_t cap_records, int32_t* out_n) {
  return debug_components(h, xyzi, offsets, n_frames, sp, true, pp, d_scratch, frame, out_records, cap_records, out_n);
}

int32_t ilcc_extract_auto_batch(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames, const ilcc_seed_params* sp,
                                ilcc_result* out, float* out_seed, int32_t* out_rank) {
  return extract_auto_batch(h, xyzi, offsets, n_frames, sp, false, nullptr, out, out_seed, out_rank);
}
int32_t ilcc_extract_auto_planar_batch(ilcc_handle* h, const float* xyzi, const uint64_t* offsets, uint32_t n_frames, const ilcc_seed_params* sp,
                                       const ilcc_seed_planar_params* pp, ilcc_result* out, float* out_seed, int32_t* out_rank) {
  return extract_auto_batch(h, xyzi, offsets, n_frames, sp, true, pp, out, out_seed, out_rank);
}

int32_t ilcc_extract_auto(ilcc_handle* h, const float* xyzi, uint32_t n, const ilcc_seed_params* sp, ilcc_result* out, float out_seed[3],
                          int32_t* out_rank) {
  const uint64_t off[2] = {0, n};
  return extract_auto_batch(h, xyzi, off, 1, sp, false, nullptr, out, out_seed, out_rank);
}
int32_t ilcc_extract_auto_planar(ilcc_handle* h, const float* xyzi, uint32_t n, const ilcc_seed_params* sp, const ilcc_seed_planar_params* pp,
                                 ilcc_result* out, float out_seed[3], int32_t* out_rank) {
  const uint64_t off[2] = {0, n};
  return extract_auto_batch(h, xyzi, off, 1, sp, true, pp, out, out_seed, out_rank);
}

}  // extern "C"
