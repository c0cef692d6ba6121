// K6 locate: where the minimum is and the frame's bound, in front of the full pass (k6_grid_cost.hip) -- k6_locate (seed +
// refinement + anchor in one launch) and k6_anchor (one anchor round of the separate launches)
#include "k6_common.h"

#ifdef ILCC_K6_TIMING
#include <algorithm>
#include <vector>
#endif

namespace ilcc {

// -DILCC_K6_TIMING: k6_locate's phases per wavefront (cycle counter stamps at the barriers between them), one record per wavefront
// in k6_locate_prof[], summed and read back through ilcc_debug_k6_locate_profile (tools/dev_locate_phases.py) -- the full pass's
// counterpart is in k6_grid_cost.hip
#ifdef ILCC_K6_TIMING
constexpr int kLocateProfWaves = 1 << 14, kLocateProfWords = 8;
__device__ unsigned long long k6_locate_prof[kLocateProfWaves * kLocateProfWords];
#define K6L_STAMP(name) const unsigned long long name = __builtin_readcyclecounter()
#else
#define K6L_STAMP(name)
#endif

// Where anchor_walk reads walk position `at` of the frame from: load() fetches the raw point and its label as the source keeps it,
// hw() turns that label into 0.5 * (label == white) once the loads of a batch of trips are all issued.
// WalkStaged: the whole walk layout of the frame, staged in LDS by k6_locate (the label already as 0.5 * white).
struct WalkStaged {
  using Label = float;
  const float2* yz;
  const float* half_white;
  __device__ __forceinline__ void load(uint32_t at, float2& v, Label& l) const {
    v = yz[at];
    l = half_white[at];
  }
  __device__ __forceinline__ float hw(Label l) const { return l; }
};
// WalkGlobal: the frame's arrays in global memory (k6_anchor; frames k6_locate cannot stage).  LAYOUT: the walk layout, where a walk
// over ALL points reads position `at` at index `at` (layout_source with n_in == Mi_all and n_rm == n_rim_all is the identity); else the
// frame's own arrays in golden-ratio order.
template <bool LAYOUT>
struct WalkGlobal {
  using Label = uint8_t;
  const float2* __restrict__ yz;
  const uint8_t* __restrict__ lab;
  uint32_t M, S;
  __device__ __forceinline__ explicit WalkGlobal(const FrameWalk& fw) : yz(fw.yz), lab(fw.lab), M(fw.M), S(fw.S) {}
  __device__ __forceinline__ void load(uint32_t at, float2& v, Label& l) const {
    const uint32_t src = LAYOUT ? at : (uint32_t)(((uint64_t)at * S) % M);
    v = yz[src];
    l = lab[src];
  }
  __device__ __forceinline__ float hw(Label l) const { return l ? 0.5f : 0.f; }
};

// ANCHOR (k6_anchor, and the last stage of k6_locate): the 4 x 4 tile at (a_org, b_org) of the full tables t at theta k on EVERY
// labelled point of the frame (M of them, the first Mi_all interior class), by the n_parts wavefronts of that theta -- blocks of four
// walk positions go round them, this one takes blocks part, part + n_parts, ...  Writes the quad sums of its 16 candidates (cost / 2 per
// phase) to s_part[candidate][phase].  ty / tz: the translation tables (in LDS or in global memory).
// A lane adds the terms of walk positions part * 4 + slice + 4 n_parts t, t ascending -- the order the published bound depends on --
// in three stretches that need no test per trip: the trips whose four positions are all interior class, the trips whose four are all
// border class, and between and behind them at most one trip each that tests every lane (Mi_all inside the quad; the last,
// incomplete quad).  The loads of kAnchorAhead trips are issued before the first of their terms is computed.
constexpr int kAnchorAhead = 4;
template <class Source>
__device__ __forceinline__ void anchor_walk(const ilcc_params& p, const GridTables& t, const Source& src, uint32_t M, uint32_t Mi_all, int k, int a_org, int b_org,
                                            const float* ty, const float* tz, uint32_t part, uint32_t n_parts, float (*s_part)[2], uint32_t& pts_done,
                                            uint32_t& pts_in) {
  const int my_s = lane_id() & (kSlices - 1), my_c = lane_id() >> 2;
  const float Wh = 0.5f * (float)p.board_w, Hh = 0.5f * (float)p.board_h, delta2 = (float)p.huber_delta;
  const float cth = t.cth[k], sth = t.sth[k];
  const float ay = ty[min(a_org + (my_c >> 2), t.n_ty - 1)], az = tz[min(b_org + (my_c & 3), t.n_tz - 1)];
  float A0 = 0.f, A1 = 0.f;
  const uint32_t first = part * kSlices, stride = n_parts * kSlices;
  // trips of this wavefront (trip t: the quad at first + t * stride) that start below walk position x
  auto trips_below = [&](uint32_t x) { return x > first ? (x - first + stride - 1u) / stride : 0u; };
  const uint32_t n_in = trips_below(Mi_all & ~(uint32_t)(kSlices - 1));            // [0, n_in): four interior-class positions
  const uint32_t n_mix = trips_below(Mi_all);                                       // [n_in, n_mix): Mi_all inside the quad
  const uint32_t n_bd = max(n_mix, trips_below(M & ~(uint32_t)(kSlices - 1)));      // [n_mix, n_bd): four border-class positions
  const uint32_t n_all = trips_below(M);                                            // [n_bd, n_all): the incomplete quad
  auto term = [&](auto interior, const float2 raw, float hw) {
    const float2 v = rotate(raw, cth, sth);
    const PointTerms pt{v.x, v.y, hw};
    if constexpr (decltype(interior)::value)
      accumulate_interior(pt, ay, az, delta2, A0, A1);
    else
      accumulate<true>(pt, ay, az, Wh, Hh, delta2, A0, A1);
  };
  // trips [t0, t1), every position of them valid and of one class
  auto whole_trips = [&](uint32_t t0, uint32_t t1, auto interior) {
    uint32_t tr = t0;
    for (; tr + (uint32_t)kAnchorAhead <= t1; tr += kAnchorAhead) {
      float2 v[kAnchorAhead];
      typename Source::Label l[kAnchorAhead];
#pragma unroll
      for (int e = 0; e < kAnchorAhead; ++e) src.load(first + (tr + (uint32_t)e) * stride + (uint32_t)my_s, v[e], l[e]);
#pragma unroll
      for (int e = 0; e < kAnchorAhead; ++e) term(interior, v[e], src.hw(l[e]));
    }
    if (tr < t1) {   // (the last 1 ... kAnchorAhead - 1: the same batch of loads, the spare ones on the last trip again)
      float2 v[kAnchorAhead - 1];
      typename Source::Label l[kAnchorAhead - 1];
#pragma unroll
      for (int e = 0; e < kAnchorAhead - 1; ++e) src.load(first + min(tr + (uint32_t)e, t1 - 1u) * stride + (uint32_t)my_s, v[e], l[e]);
#pragma unroll
      for (int e = 0; e < kAnchorAhead - 1; ++e)
        if (tr + (uint32_t)e < t1) term(interior, v[e], src.hw(l[e]));   // (wave-uniform)
    }
  };
  // trips [t0, t1) -- at most one -- whose lanes each test their own position
  auto tested_trips = [&](uint32_t t0, uint32_t t1) {
    for (uint32_t tr = t0; tr < t1; ++tr) {
      const uint32_t at = first + tr * stride + (uint32_t)my_s;
      if (at < M) {
        float2 v;
        typename Source::Label l;
        src.load(at, v, l);
        if (at < Mi_all)
          term(std::true_type{}, v, src.hw(l));
        else
          term(std::false_type{}, v, src.hw(l));
      }
    }
  };
  whole_trips(0u, n_in, std::true_type{});
  tested_trips(n_in, n_mix);
  whole_trips(n_mix, n_bd, std::false_type{});
  tested_trips(n_bd, n_all);
  pts_done += n_all * (uint32_t)kSlices;
  pts_in += n_mix * (uint32_t)kSlices;
  const float t0s = quad_sum(A0), t1s = quad_sum(A1);
  if (my_s == 0) {
    s_part[my_c][0] = t0s;
    s_part[my_c][1] = t1s;
  }
}
// the walk of a frame that is not staged: through its layout in global memory, or (no layout) its own arrays
template <class... Rest>
__device__ __forceinline__ void anchor_walk_global(const ilcc_params& p, const GridTables& t, const FrameWalk& fw, Rest&&... rest) {
  if (fw.layout)
    anchor_walk(p, t, WalkGlobal<true>(fw), fw.M, fw.Mi_all, rest...);
  else
    anchor_walk(p, t, WalkGlobal<false>(fw), fw.M, 0u, rest...);
}

// The anchor's result, by one wavefront behind the barrier that follows the walks: candidate (t, cand) costs the sum of its PARTS
// partial sums s_part[t * PARTS + part][cand], in part order (the published bound is compared bit for bit downstream); the argmin over
// (theta k0 + th, candidate) of the tables t carries (a << 16) | b.  Lane 0 writes the record and lowers the frame's bound word: a complete candidate on
// every point is a valid bound.
template <int THETAS, int PARTS>
__device__ __forceinline__ void anchor_publish(const GridTables& t, uint32_t* bound, const float (*s_part)[16][2], int k0, int a_org, int b_org,
                                               GridPartial* out) {
  const int lane = lane_id();
  const int n_ty = t.n_ty, n_tz = t.n_tz;
  Best best{__builtin_inff(), 0xFFFFFFFFu, 0xFFFFFFFFu};
  uint32_t ab = 0;
  if (lane < 16 * THETAS) {
    const int th = lane >> 4, cand = lane & 15;
    const int k = min(max(k0 + th, 0), t.n_th - 1), ja = a_org + (cand >> 2), jb = b_org + (cand & 3);
    if (ja < n_ty && jb < n_tz) {
      float h0 = 0.f, h1 = 0.f;
#pragma unroll
      for (int q = 0; q < PARTS; ++q) {
        h0 += s_part[th * PARTS + q][cand][0];
        h1 += s_part[th * PARTS + q][cand][1];
      }
      score(2.f * h0, 2.f * h1, k, ja, jb, n_ty, n_tz, t.c_th, t.c_ty, t.c_tz, best, ab);
    }
  }
  best = wave_argmin<true>(best, ab);
  if (lane == 0) {
    *out = GridPartial{best.cost, best.d2, best.flat, ab};
    if (best.flat != 0xFFFFFFFFu) atomicMin(bound, __float_as_uint(best.cost));
  }
}

// k6_locate (round 5): seed + refinement + anchor in ONE launch, one workgroup per frame.  The three launches it replaces only
// have to say WHERE the minimum is and publish the frame's bound; as 17 small workgroups per frame in three dependent launches
// they were 277 of the K6 stage's 733 us with a batch alone on the chip, at 16-28 % issue utilisation: each stages
// its points and tables again, reads the previous launch's argmin from global memory, and the anchor's workgroups run one
// wavefront of four.  Here a frame's 6 wavefronts
//   1. stage the SAMPLE of the walk (an eighth of the labelled points, a proportional prefix of each class of the walk layout)
//      once, rotated by the five seed thetas; 5 x (8 x 8 decimated translations) = 20 tiles, one per wavefront at a time,
//      pruned against a bound word in LDS; argmin in LDS;
//   2. rotate the sample by the (2 r + 1) thetas around the seed's and score their 8 x 8 windows of full-table translations
//      (kLocateWindowTiles; 36 tiles); argmin in LDS;
//   3. score the 4 x 4 tile around that argmin at theta - 1, theta, theta + 1 on EVERY labelled point (rotated on the fly from
//      the walk layout, which all six first copy from L2 into the LDS the rotated sample no longer needs -- round 13; until then
//      every trip of the walk was a round trip to L2), two wavefronts per theta on alternate blocks of the walk, and publish the
//      best complete cost as the frame's bound and its candidate as the full pass's starting tile.
// Same on both paths: the final results.  The full pass is exact for any bound it is given -- the bound only has to be the cost of
// SOME complete candidate, and a candidate is cut, or listed as a near tie, with 2e-5 to spare (20 x the rounding of an fp32 sum of a
// thousand terms).  Not the same: this path keeps the 8 x 8 refinement window on grids whose seed stride is wider than 8 translations
// (the separate launches widen theirs to 16 x 16 there) and runs one anchor round, against kAnchorRounds; its anchor also adds two
// parts of the walk per theta where k6_anchor adds eight.  So the bound it publishes, and the full pass's executed work, can differ.
// Batches of fewer than kLocateMinFrames frames keep the separate launches: there a frame's 17 workgroups are what fills the chip.
constexpr int kLocateThreads = 384;       // 6 wavefronts = 3 anchor thetas x 2 parts of the walk, all busy in the anchor.  Measured (k frames/s / locate alone): 256: 1056, 512: 1089, 1024: 1011-1033 when it was built; on the final build 384: 1266 / 0.184 ms, 512: 1268 / 0.214 ms, 768: 1251 / 0.201 ms
constexpr int kSeedPeek = 16;             // walk positions of every seed tile a wavefront looks at before it chooses which tile to evaluate first
constexpr int kAnchorThetas = 3;          // thetas around the refinement's argmin the anchor scores (1: locate 0.26 -> 0.21 ms alone, full pass 0.36 -> 0.40: a wash)
constexpr int kAnchorParts = (kLocateThreads / 64) / kAnchorThetas;  // wavefronts sharing a theta's walk
constexpr int kLocateWaves = kLocateThreads / ILCC_WAVE;
constexpr int kLocateThetasMax = 16;      // rotations of the sample kept in LDS at a time (seed: 5, refinement: 2 r + 1 = 9).  Round 13, a region of the 9 this grid uses (37 -> 25 KB per workgroup): bench 1 366 -> 1 372 k frames/s, locate's pipelined average 335 -> 329 us -- inside the noise, not kept
constexpr int kStageAhead = 8;            // anchor staging: loads a thread issues before its first LDS write (1 792 points: 5 per thread)
// k6_locate's refinement window, in tiles per axis: 2 (8 x 8 translations around the seed's argmin) on EVERY grid.  The separate
// launches widen theirs to 4 tiles (16 x 16) on grids whose seed stride is wider than 8 translations (GridPass::window_tiles); whether
// this path should too is a change of its own, to be measured.
constexpr int kLocateWindowTiles = 2;

// k6_locate's dynamic LDS as byte offsets: the raw sample (sample_cap float2, at 0), its labels (sample_cap float 0.5 * white), the
// region of its kLocateThetasMax rotations (float2 each) -- which the anchor, once the refinement is through with it, fills with the
// frame's whole walk layout (stage_cap float2 at rot, stage_cap float 0.5 * white at stage_hw), so the region is at least that
// large; with LocatePlan's capacities it never has to grow for it: 12 stage_cap <= 16 x 8 sample_cap bytes, sample_cap being at
// least stage_cap / 8 -- then the (ty, tz) tables -- the full ones, then the seed's -- and the total.  The kernel carves with these
// offsets and locate_lds_bytes returns the total.
struct LocateLds {
  size_t hw, rot, stage_hw, ay, az, ay2, az2, bytes;
};
__host__ __device__ constexpr LocateLds locate_lds(uint32_t sample_cap, uint32_t stage_cap, int n_ty, int n_tz, int n_ty2, int n_tz2) {
  LocateLds l{};
  l.hw = sizeof(float2) * (size_t)sample_cap;
  l.rot = l.hw + sizeof(float) * (size_t)sample_cap;
  l.stage_hw = l.rot + sizeof(float2) * (size_t)stage_cap;
  const size_t rotations = sizeof(float2) * (size_t)kLocateThetasMax * sample_cap, staged = (sizeof(float2) + sizeof(float)) * (size_t)stage_cap;
  l.ay = l.rot + (rotations > staged ? rotations : staged);
  l.az = l.ay + sizeof(float) * (size_t)n_ty;
  l.ay2 = l.az + sizeof(float) * (size_t)n_tz;
  l.az2 = l.ay2 + sizeof(float) * (size_t)n_ty2;
  l.bytes = l.az2 + sizeof(float) * (size_t)n_tz2;
  return l;
}
size_t locate_lds_bytes(const LocatePlan& lp, int n_ty, int n_tz) {
  return locate_lds(lp.sample_cap, lp.stage_cap, n_ty, n_tz, lp.seed.n_ty, lp.seed.n_tz).bytes;
}

__global__ __launch_bounds__(kLocateThreads) void k6_locate(Ctx c, LocatePlan lp) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ Best s_best[kLocateWaves];
  __shared__ uint32_t s_ab[kLocateWaves];
  __shared__ uint32_t s_bound;              // float bits: best complete SAMPLE cost so far (seed and refinement share the sample)
  __shared__ uint32_t s_pick[4];            // argmin of a phase: flat, (a << 16) | b
  __shared__ uint32_t s_iters[kLocateWaves], s_iters_in[kLocateWaves];
  __shared__ float s_part[kAnchorThetas * kAnchorParts][16][2];     // anchor: (theta, part of the walk) -> (candidate, phase) partial costs / 2
  const uint32_t f = blockIdx.x;
  GridPartial* out = lp.out + f;
  K6L_STAMP(t_entry);
  const int lane = lane_id();
  const int wid = __builtin_amdgcn_readfirstlane(wave_id());
  if (c.res[f].status != ILCC_OK) {
    if (threadIdx.x == 0) no_candidate(out);
    return;
  }
  const FrameWalk fw(c, f);
  const uint32_t Ms = min(fw.sample(lp.sample_min), lp.sample_cap);
  uint32_t n_in, n_rm;
  fw.prefix(Ms, n_in, n_rm);
  const GridTables& full = c.grid;   // (the seed scores lp.seed, refinement and anchor the full tables)
  const int n_ty = full.n_ty, n_tz = full.n_tz, n_th = full.n_th;
  const int n_ty2 = lp.seed.n_ty, n_tz2 = lp.seed.n_tz;
  const LocateLds l = locate_lds(lp.sample_cap, lp.stage_cap, n_ty, n_tz, n_ty2, n_tz2);
  float2* s_raw = reinterpret_cast<float2*>(smem);
  float* s_hw = lds_next<float>(s_raw, 0, l.hw);
  float2* s_rot = lds_next<float2>(s_hw, l.hw, l.rot);   // [kLocateThetasMax][sample_cap]; behind the refinement [stage_cap] points of the walk layout ...
  float* s_stage_hw = lds_next<float>(s_rot, l.rot, l.stage_hw);   // ... and their [stage_cap] labels
  float* s_ay = lds_next<float>(s_rot, l.rot, l.ay);
  float* s_az = lds_next<float>(s_ay, l.ay, l.az);
  float* s_ay2 = lds_next<float>(s_az, l.az, l.ay2);
  float* s_az2 = lds_next<float>(s_ay2, l.ay2, l.az2);
  for (uint32_t sl = threadIdx.x; sl < Ms; sl += kLocateThreads) {
    const uint32_t src = fw.source(sl, n_in, n_rm);
    s_raw[sl] = fw.yz[src];
    s_hw[sl] = fw.lab[src] ? 0.5f : 0.f;
  }
  for (int i = threadIdx.x; i < n_ty; i += kLocateThreads) s_ay[i] = full.ay[i];
  for (int i = threadIdx.x; i < n_tz; i += kLocateThreads) s_az[i] = full.az[i];
  for (int i = threadIdx.x; i < n_ty2; i += kLocateThreads) s_ay2[i] = lp.seed.ay[i];
  for (int i = threadIdx.x; i < n_tz2; i += kLocateThreads) s_az2[i] = lp.seed.az[i];
  if (threadIdx.x == 0) s_bound = 0x7f800000u;
  const float Wh = 0.5f * (float)c.p.board_w, Hh = 0.5f * (float)c.p.board_h, delta2 = (float)c.p.huber_delta;
  const int my_s = lane & (kSlices - 1), my_c = lane >> 2, my_a = my_c >> 2, my_b = my_c & 3;
  uint32_t pts_done = 0, pts_in = 0;

  // the sample rotated by n_rot thetas (theta index of rotation r: th_of(r))
  auto rotate_sample = [&](int n_rot, auto th_of, const float* cth_tab, const float* sth_tab) {
    for (uint32_t item = threadIdx.x; item < (uint32_t)n_rot * Ms; item += kLocateThreads) {
      const uint32_t r = item / Ms, sl = item - r * Ms;
      const int k = th_of((int)r);
      s_rot[(size_t)r * lp.sample_cap + sl] = rotate(s_raw[sl], cth_tab[k], sth_tab[k]);
    }
  };
  // one 4 x 4 tile on the rotated sample `rot`, quad-sliced like k6_grid_cost (border class first, a bound test every 8 walk
  // positions against the sample bound); false: every candidate provably loses
  auto sample_tile = [&](const float2* rot, float ay, float az, float& c0, float& c1) -> bool {
    float A0 = 0.f, A1 = 0.f;
    uint32_t since = 0;
    float lim2 = 0.5f * (1.f + kTieEps) * __uint_as_float(s_bound);
    uint32_t pos = 0;
    for (uint32_t at0 = n_in; at0 < Ms; at0 += kSlices) {   // (at0 is wave-uniform: every lane makes the same trips)
      const uint32_t at = at0 + (uint32_t)my_s;
      if (at < Ms) {
        const float2 v = rot[at];
        accumulate<true>(PointTerms{v.x, v.y, s_hw[at]}, ay, az, Wh, Hh, delta2, A0, A1);
      }
      pos += kSlices;
      since += kSlices;
      if (since >= 8u) {
        since = 0;
        const float part = fminf(quad_sum(A0), quad_sum(A1));
        if (__ballot(!(part > lim2)) == 0ull) {
          pts_done += pos;
          return false;
        }
        lim2 = 0.5f * (1.f + kTieEps) * __uint_as_float(s_bound);
      }
    }
    for (uint32_t at0 = 0; at0 < n_in; at0 += kSlices) {
      const uint32_t at = at0 + (uint32_t)my_s;
      if (at < n_in) {
        const float2 v = rot[at];
        accumulate_interior(PointTerms{v.x, v.y, s_hw[at]}, ay, az, delta2, A0, A1);
      }
      pos += kSlices;
      since += kSlices;
      if (since >= 8u) {
        since = 0;
        const float part = fminf(quad_sum(A0), quad_sum(A1));
        if (__ballot(!(part > lim2)) == 0ull) {
          pts_done += pos;
          pts_in += at0 + kSlices;
          return false;
        }
        lim2 = 0.5f * (1.f + kTieEps) * __uint_as_float(s_bound);
      }
    }
    pts_done += pos;
    pts_in += n_in;
    c0 = 2.f * quad_sum(A0);
    c1 = 2.f * quad_sum(A1);
    return true;
  };
  // a phase's argmin: every wavefront's best -> LDS -> s_pick (flat, ab)
  auto reduce_best = [&](Best best, uint32_t ab) {
    best = wave_argmin<true>(best, ab);
    if (lane == 0) {
      s_best[wid] = best;
      s_ab[wid] = ab;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t bab = 0;
      const Best b = block_argmin<kLocateWaves>(s_best, s_ab, bab);
      s_pick[0] = b.flat;
      s_pick[1] = bab;
      s_pick[2] = __float_as_uint(b.cost);
      s_pick[3] = b.d2;
    }
    __syncthreads();
  };
  // a completed sample tile: the wavefront's best cost (v: this lane's) lowers the sample bound
  auto lower_sample_bound = [&](float v) {
    const float wb = wave_min(v);
    if (lane == 0) atomicMin(&s_bound, __float_as_uint(wb));   // costs are >= 0: uint order == float order
  };
  __syncthreads();
  K6L_STAMP(t_staged);

  // ---- 1. seed: n_th2 thetas x (n_ty2 x n_tz2 decimated translations) on the sample
  const int n_th2 = min(lp.seed.n_th, kLocateThetasMax);
  rotate_sample(n_th2, [&](int r) { return r; }, lp.seed.cth, lp.seed.sth);
  __syncthreads();
  {
    const int nta = axis_tiles(n_ty2), ntb = axis_tiles(n_tz2), per = nta * ntb, n_tiles = n_th2 * per;
    Best best{__builtin_inff(), 0xFFFFFFFFu, 0xFFFFFFFFu};
    uint32_t best_ab = 0;
    // The order of the tiles never changes the result (only provably losing candidates are cut, ties never), but it decides how
    // soon the sample bound is tight.  Every wavefront therefore first looks at the first kSeedPeek walk positions of each of
    // its tiles, evaluates the most promising one in full -- one of the eight is nearly always in the right basin -- and only then
    // walks the others, which now die at their first tests.
    int t_first = -1;
    {
      float peek_best = __builtin_inff();
      for (int t = wid; t < n_tiles; t += kLocateWaves) {
        const int k2 = t / per, q = t - k2 * per, ta = q / ntb, tb = q - ta * ntb;
        const int ia = ta * kTile + my_a, ib = tb * kTile + my_b;
        const float2* rot = s_rot + (size_t)k2 * lp.sample_cap;
        const float ay = s_ay2[min(ia, n_ty2 - 1)], az = s_az2[min(ib, n_tz2 - 1)];
        float A0 = 0.f, A1 = 0.f;
        for (uint32_t at0 = n_in; at0 < min(Ms, n_in + (uint32_t)kSeedPeek); at0 += kSlices) {
          const uint32_t at = at0 + (uint32_t)my_s;
          if (at < Ms) {
            const float2 v = rot[at];
            accumulate<true>(PointTerms{v.x, v.y, s_hw[at]}, ay, az, Wh, Hh, delta2, A0, A1);
          }
        }
        pts_done += min(Ms - n_in, (uint32_t)kSeedPeek);
        const float pm = wave_min((ia < n_ty2 && ib < n_tz2) ? fminf(quad_sum(A0), quad_sum(A1)) : __builtin_inff());
        if (pm < peek_best) {   // (wave-uniform)
          peek_best = pm;
          t_first = t;
        }
      }
    }
    const int n_mine = (n_tiles - wid + kLocateWaves - 1) / kLocateWaves;   // tiles of this wavefront
    for (int it = (t_first >= 0 ? -1 : 0); it < n_mine; ++it) {
      const int t = it < 0 ? t_first : wid + it * kLocateWaves;
      if (it >= 0 && t == t_first) continue;
      const int k2 = t / per, q = t - k2 * per, ta = q / ntb, tb = q - ta * ntb;
      const int ia = ta * kTile + my_a, ib = tb * kTile + my_b;
      const bool owner = ia < n_ty2 && ib < n_tz2;
      float c0, c1;
      if (!sample_tile(s_rot + (size_t)k2 * lp.sample_cap, s_ay2[min(ia, n_ty2 - 1)], s_az2[min(ib, n_tz2 - 1)], c0, c1)) continue;
      if (owner) score(c0, c1, k2, ia, ib, n_ty2, n_tz2, lp.seed.c_th, lp.seed.c_ty, lp.seed.c_tz, best, best_ab);
      lower_sample_bound(owner ? fminf(c0, c1) : __builtin_inff());
    }
    reduce_best(best, best_ab);
  }
  K6L_STAMP(t_seeded);
  if (s_pick[0] == 0xFFFFFFFFu) {   // (no candidate at all: an empty frame)
    if (threadIdx.x == 0) no_candidate(out);
    return;
  }
  // ---- 2. refinement: theta within +- refine_radius steps of the seed's, the window of full-table translations around its argmin
  const int k2s = (int)((s_pick[0] >> 1) / (uint32_t)(n_ty2 * n_tz2));
  const int sa = min((int)(s_pick[1] >> 16) * lp.map.stride_t, n_ty - 1), sbb = min((int)(s_pick[1] & 0xFFFFu) * lp.map.stride_t, n_tz - 1);
  // every OTHER theta of the refinement's range: the anchor scores theta - 1, theta, theta + 1 around its argmin on every point, so
  // the thetas in between are still looked at -- measured: locate 0.265 -> 0.229 ms alone, the full pass's time and executed work
  // unchanged (the bound is as tight), bench 1085 -> 1112 k frames/s; every fourth theta, or every other translation: no further gain
  constexpr int kRefStride = kRefineThetaStride;
  const int n_ref = min(2 * (lp.refine_radius / kRefStride) + 1, kLocateThetasMax);
  const int k_ref0 = lp.map.off_th + k2s * lp.map.stride_th - (lp.refine_radius / kRefStride) * kRefStride;
  rotate_sample(n_ref, [&](int r) { return min(max(k_ref0 + kRefStride * r, 0), n_th - 1); }, full.cth, full.sth);
  __syncthreads();
  {
    constexpr int kWindow = kLocateWindowTiles * kTile;
    const int a_org = window_origin(sa, kWindow / 2, n_ty, kWindow), b_org = window_origin(sbb, kWindow / 2, n_tz, kWindow);
    const int nta = min(kLocateWindowTiles, axis_tiles(n_ty)), ntb = min(kLocateWindowTiles, axis_tiles(n_tz));
    const int per = nta * ntb, n_tiles = n_ref * per;
    Best best{__builtin_inff(), 0xFFFFFFFFu, 0xFFFFFFFFu};
    uint32_t best_ab = 0;
    for (int t = wid; t < n_tiles; t += kLocateWaves) {
      const int r = t / per, q = t - r * per, ta = q / ntb, tb = q - ta * ntb;
      const int k = min(max(k_ref0 + kRefStride * r, 0), n_th - 1);
      const int ia = a_org + ta * kTile + my_a, ib = b_org + tb * kTile + my_b;
      const bool owner = ia < n_ty && ib < n_tz;
      float c0, c1;
      if (!sample_tile(s_rot + (size_t)r * lp.sample_cap, s_ay[min(ia, n_ty - 1)], s_az[min(ib, n_tz - 1)], c0, c1)) continue;
      if (owner) score(c0, c1, k, ia, ib, n_ty, n_tz, full.c_th, full.c_ty, full.c_tz, best, best_ab);
      lower_sample_bound(owner ? fminf(c0, c1) : __builtin_inff());
    }
    reduce_best(best, best_ab);
  }
  K6L_STAMP(t_refined);
  // ---- 3. anchor: the 4 x 4 tile around the refinement's argmin at theta - 1, theta, theta + 1 on EVERY labelled point
  {
    // (the refinement evaluates every candidate of the seed's argmin window again, so it always has a pick)
    const int kr = (int)((s_pick[0] >> 1) / (uint32_t)(n_ty * n_tz));
    const int ra = min((int)(s_pick[1] >> 16), n_ty - 1), rb = min((int)(s_pick[1] & 0xFFFFu), n_tz - 1);
    const int a_org = window_origin(ra, 1, n_ty, kTile), b_org = window_origin(rb, 1, n_tz, kTile);
    const int k0 = kr - kAnchorThetas / 2;
    // The region of the rotated sample is dead behind the refinement's reduce_best: a frame whose walk layout fits gets it staged
    // there, raw, by all threads with coalesced loads -- a thread's loads (kStageAhead at a time) all issued before its first LDS
    // write -- and the anchor's wavefronts walk LDS.  Other frames (more than stage_cap points, or no layout) walk global memory.
    const bool staged = fw.layout && fw.M <= lp.stage_cap;   // (uniform over the workgroup)
    if (staged) {
      auto stage = [&](uint32_t base, auto ahead) {
        constexpr int N = decltype(ahead)::value;
        float2 v[N];
        uint8_t lb[N];
#pragma unroll
        for (int e = 0; e < N; ++e) {
          const uint32_t i = min(base + (uint32_t)e * kLocateThreads + threadIdx.x, fw.M - 1u);
          v[e] = fw.yz[i];
          lb[e] = fw.lab[i];
        }
#pragma unroll
        for (int e = 0; e < N; ++e) {
          const uint32_t i = base + (uint32_t)e * kLocateThreads + threadIdx.x;
          if (i < fw.M) {
            s_rot[i] = v[e];
            s_stage_hw[i] = lb[e] ? 0.5f : 0.f;
          }
        }
      };
      for (uint32_t base = 0; base < fw.M; base += (uint32_t)kStageAhead * kLocateThreads) {
        if (fw.M - base <= (uint32_t)(kStageAhead / 2) * kLocateThreads)
          stage(base, std::integral_constant<int, kStageAhead / 2>{});
        else
          stage(base, std::integral_constant<int, kStageAhead>{});
      }
      __syncthreads();
    }
    K6L_STAMP(t_copied);
    if (wid < kAnchorThetas * kAnchorParts) {
      const int t = wid % kAnchorThetas, part = wid / kAnchorThetas, k = min(max(k0 + t, 0), n_th - 1);
      float(*my_part)[2] = s_part[t * kAnchorParts + part];
      if (staged)
        anchor_walk(c.p, full, WalkStaged{s_rot, s_stage_hw}, fw.M, fw.Mi_all, k, a_org, b_org, s_ay, s_az, (uint32_t)part, (uint32_t)kAnchorParts, my_part, pts_done,
                    pts_in);
      else
        anchor_walk_global(c.p, full, fw, k, a_org, b_org, s_ay, s_az, (uint32_t)part, (uint32_t)kAnchorParts, my_part, pts_done, pts_in);
    }
    __syncthreads();
    if (wid == 0) anchor_publish<kAnchorThetas, kAnchorParts>(full, c.grid_bound + f, s_part, k0, a_org, b_org, out);
#ifdef ILCC_K6_TIMING
    if (lane == 0) {   // (the record ends here: only the evaluation counters follow)
      const unsigned long long t_anchored = __builtin_readcyclecounter();
      unsigned long long* o = k6_locate_prof + (size_t)((f * kLocateWaves + (uint32_t)wid) & (kLocateProfWaves - 1)) * kLocateProfWords;
      o[0] = 1ull;
      o[1] = t_staged - t_entry;
      o[2] = t_seeded - t_staged;
      o[3] = t_refined - t_seeded;
      o[4] = t_copied - t_refined;
      o[5] = t_anchored - t_copied;
      o[6] = t_anchored - t_entry;
    }
#endif
  }
  if (lane == 0) {
    s_iters[wid] = pts_done;
    s_iters_in[wid] = pts_in;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t it_sum = 0, in_sum = 0;
    for (int w = 0; w < kLocateWaves; ++w) {
      it_sum += s_iters[w];
      in_sum += s_iters_in[w];
    }
    count_evals(c.grid_iters, f, kEvalsAll, it_sum);
    count_evals(c.grid_iters, f, kEvalsInterior, in_sum);
  }
}

// k6_anchor (round 5): one ANCHOR round for batches that keep the separate locate launches (fewer than kLocateMinFrames frames:
// BASELINE config 5's 64-frame batches).  Workgroup = (theta - 1 | theta | theta + 1 around the previous launch's argmin, frame);
// its 8 wavefronts split the walk over ALL labelled points of ONE 4 x 4 tile of translations around that argmin (blocks of
// four walk positions go round the wavefronts, partial sums meet in LDS), where the anchor instance of k6_grid_cost walked the
// tile with one wavefront of eight: 0.16 ms per round on config 5, latency of a serial walk over 4 400 points.  At 0.03 ms a
// round can be repeated: every round re-centres the tile on the previous round's argmin -- a greedy descent on complete costs
// towards the grid minimum.  On a fine grid (config 5: steps of 1.6 mm and 0.25 degrees) the refinement's argmin, found on an
// eighth of the points, is several steps from it; a second round makes the bound 20 % tighter in executed work (225 -> 180 M
// point-candidate evaluations per 64 frames in the full pass, 224 -> 189 M in the pre-passes).
constexpr int kAnchorThreads = 512;
constexpr int kAnchorWaves = kAnchorThreads / ILCC_WAVE;
__global__ __launch_bounds__(kAnchorThreads) void k6_anchor(Ctx c, GridPass pass) {
  __shared__ float s_part[kAnchorWaves][16][2];
  __shared__ uint32_t s_iters[kAnchorWaves], s_iters_in[kAnchorWaves];
  const uint32_t f = blockIdx.y, kblk = blockIdx.x;
  GridPartial* out = &pass.out[(uint64_t)f * pass.blocks + kblk];
  const int lane = lane_id();
  const int wid = __builtin_amdgcn_readfirstlane(wave_id());
  uint32_t k2u = 0, ab = 0;
  Best sb{__builtin_inff(), 0xFFFFFFFFu, 0xFFFFFFFFu};
  if (c.res[f].status == ILCC_OK) sb = seed_argmin(pass.seed, f, k2u, ab);
  if (sb.flat == 0xFFFFFFFFu) {
    if (threadIdx.x == 0) no_candidate(out);
    return;
  }
  const int n_ty = pass.t.n_ty, n_tz = pass.t.n_tz;
  const int kr = (int)((sb.flat >> 1) / (uint32_t)(n_ty * n_tz));   // (the records come from launches over the full tables)
  const int k0 = kr + (int)kblk - pass.radius_th;                      // this workgroup's theta, before the clamp to the table
  const int ra = min((int)(ab >> 16), n_ty - 1), rb = min((int)(ab & 0xFFFFu), n_tz - 1);
  const int a_org = window_origin(ra, 1, n_ty, kTile), b_org = window_origin(rb, 1, n_tz, kTile);
  uint32_t pts_done = 0, pts_in = 0;
  anchor_walk_global(c.p, pass.t, FrameWalk(c, f), min(max(k0, 0), pass.t.n_th - 1), a_org, b_org, pass.t.ay, pass.t.az, (uint32_t)wid, (uint32_t)kAnchorWaves, s_part[wid],
                     pts_done, pts_in);
  if (lane == 0) {
    s_iters[wid] = pts_done;
    s_iters_in[wid] = pts_in;
  }
  __syncthreads();
  if (wid == 0) anchor_publish<1, kAnchorWaves>(pass.t, pass.bound + f, s_part, k0, a_org, b_org, out);
  if (threadIdx.x == 0) {
    uint32_t it_sum = 0, in_sum = 0;
    for (int w = 0; w < kAnchorWaves; ++w) {
      it_sum += s_iters[w];
      in_sum += s_iters_in[w];
    }
    count_evals(c.grid_iters, f, kEvalsAll, it_sum);
    count_evals(c.grid_iters, f, kEvalsInterior, in_sum);
  }
}

void launch_anchor(const Ctx& c, const GridPass& pass, hipStream_t s) {
  hipLaunchKernelGGL(k6_anchor, dim3(pass.blocks, c.n_frames), dim3(kAnchorThreads), 0, s, c, pass);
}

void launch_locate(const Ctx& c, hipStream_t s, const LocatePlan& lp) {
  const size_t lds = locate_lds_bytes(lp, c.grid.n_ty, c.grid.n_tz);
  hipLaunchKernelGGL(k6_locate, dim3(c.n_frames), dim3(kLocateThreads), lds, s, c, lp);
}

#ifdef ILCC_K6_TIMING
// out8: wavefronts recorded, then their summed cycles of staging, seed, refinement, the anchor's copy to LDS, the anchor's walk and
// result (to the barrier behind it and wavefront 0's publish), and of the whole life up to there
extern "C" int ilcc_debug_k6_locate_profile(unsigned long long* out8, int clear) {
  static std::vector<unsigned long long> host((size_t)kLocateProfWaves * kLocateProfWords);
  if (hipMemcpyFromSymbol(host.data(), HIP_SYMBOL(k6_locate_prof), host.size() * sizeof(unsigned long long)) != hipSuccess) return -1;
  for (int k = 0; k < kLocateProfWords; ++k) out8[k] = 0;
  for (size_t w = 0; w < (size_t)kLocateProfWaves; ++w)
    for (int k = 0; k < kLocateProfWords; ++k) out8[k] += host[w * kLocateProfWords + k];
  if (clear) {
    std::fill(host.begin(), host.end(), 0ull);
    if (hipMemcpyToSymbol(HIP_SYMBOL(k6_locate_prof), host.data(), host.size() * sizeof(unsigned long long)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

hipError_t set_kernel_attributes_k6_locate() { return raise_grid_lds_limit({(const void*)k6_locate}); }

}  // namespace ilcc
