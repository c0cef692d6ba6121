// K6 grid_cost -- the hot kernel.  Evaluates the ILCC intensity-grid objective of
// Optimization::get_theta_t (/root/reference/ilcc2/src/Optimization.cpp:94-160), i.e.
//     cost(theta,ty,tz,phase) = 1/2 * sum_k HuberLoss(0.1)( r_k^2 ),
// r_k = VirtualboardError::operator() (/root/reference/ilcc2/include/ilcc2/Optimization.h:31-107)
// for EVERY candidate of an exhaustive (theta, ty, tz) x colour-phase grid (the reference only
// walks this surface locally with Ceres from (0,0,0)).
//
// (Round 4: k6_group_prepass (k6_group_prepass.hip) runs ONE such pre-pass for five consecutive thetas in front of the full pass; a
// full-pass workgroup starts from its group's rejected-tile mask, or exits at once when the group left no tile.)
// Mapping (gfx950): workgroup = (frame, theta index), 4 wavefronts (8 on frames staged above 2048 points).  The frame's
// labelled points are rotated by the workgroup's theta and staged ONCE into LDS.  A wavefront owns a tile of
// 4 x 4 (ty, tz) candidates; lane = candidate * 4 + slice: the four lanes of a quad evaluate the SAME
// candidate on four interleaved quarters of the point walk and keep private running sums (both
// colour phases).  The branch-and-bound test therefore needs only a quad reduction -- four DPP adds --
// and runs every 8 positions of the walk (2 points per lane): a tile stops the moment each of its candidates is provably
// beaten.  The walk starts with the border-class points closest to the board's outline (rim), then the other border-class
// points, then the interior-class ones -- the layout k5w_walk_order (k5w_walk_order.hip) writes once per frame.  Before any
// tile is started, the full pass runs a BOX PRE-PASS: a lower bound for all 16 candidates of a tile from the out-of-board
// cost of 32 rim points at the tile's extreme translations (box_term); 93-99 % of the tiles are never started.  The first
// block of the walk lives in registers (DESIGN.md section 4 has the measurements behind every one of these choices).
// History of this mapping, measured on the 128-frame batch:
//  * lanes = points, 4 x 4 candidates in registers (round-1 first design): 14.5 VALU per evaluation
//    thanks to separable i/j terms, but every test needed a ~130-instruction transposed reduction over
//    32 accumulators and could only run at 1/16, 1/8, 1/4, 1/2 of the points: >= 400 instructions per
//    tile however hopeless the tile (2.8 M wave-instructions per frame, 0.89 ms per batch);
//  * one candidate per lane, 8 x 8 tiles: no reduction at all, but a surviving tile is a serial walk over
//    all M points by ONE wavefront (~50 us): the launch tails dominated (1.05 ms);
//  * this one: quad-sliced -- a quarter of the serial length, 4 x 4 pruning granularity.
// No MFMA: there is no dense contraction.  The cost volume is never written (in-kernel argmin)
// unless the diagnostic entry asks for it.
//
// Per point and candidate, with i = (y' + ty + W g/2)/g, j likewise (Optimization.h:45-46):
//   in board (0<i<W, 0<j<H):  r = dist(i, nearest integer) + dist(j, nearest integer) when the
//                             cell colour differs from the point's label, else 0   (:50-83)
//   out of board:             r = min(|i|,|i-W|) + min(|j|,|j-H|) if useOutofBoard    (:85-104)
//   1/2 rho(r^2) = q (r - q/2),  q = min(r, delta)                     (HuberLoss(0.1), :137)
// The cell is white iff topleftWhite xor ((floor i + floor j) odd)  (:53-61), so a mismatch
// under phase 0 is a match under phase 1: both phases come out of one pass.
// A lane's sums carry cost / 2 (the colour weight is 0 or 1/2; powers of two, exact): 29 VALU
// instructions per point and lane for a border-class point (out-of-board logic included; 26 inside the unrolled walk), 15
// for an interior-class point (it is in the board under every translation of the grid: accumulate_interior) --
// tools/k6_isa_count.sh counts them in the assembly of the probe kernels at the end of this file.
#include "k6_common.h"
#ifdef ILCC_K6_TIMING
#include <algorithm>
#include <vector>
#endif

namespace ilcc {

// -DILCC_K6_TIMING: per-wavefront cycle budget of the FULL pass (s_memtime around the phases of a workgroup's life), summed
// into k6_prof[] and read back through ilcc_debug_k6_profile (tools/dev_k6_timing.py).  Costs ~10 % of the kernel's time.
#ifdef ILCC_K6_TIMING
constexpr int kProfWaves = 1 << 17, kProfWords = 16;
__device__ unsigned long long k6_prof[kProfWaves * kProfWords];   // one record per wavefront: plain stores, no atomics
#define K6_NOW() __builtin_readcyclecounter()
#else
#define K6_NOW() 0ull
#endif

// The workgroup's own box pre-pass over its n_tiles tiles (see grid_cost_body): s_dead starts from the common pre-pass's mask s_dead0
// when there is one -- and stays that: behind a valid mask the workgroup runs no rounds of its own -- else from zero, and gets the
// bits of the tiles whose bound on the n_pre sample points s_ij[Mi ...] exceeds the frame's bound gb_bits.  Returns whether a tile
// is left alive; adds the (point, tile) evaluations to box_evals.  Uses s_cnt[0 .. 2] and s_iters; ends behind a barrier.
template <int THREADS>
__device__ __forceinline__ bool own_box_prepass(int n_tiles, int ntb, int a_org, int b_org, int n_ty, int n_tz, const float* s_ay, const float* s_az,
                                                const float2* s_ij, uint32_t Mi, uint32_t n_pre, uint32_t gb_bits, const uint32_t* s_dead0, uint32_t* s_dead,
                                                uint16_t* s_live, uint32_t* s_cnt, uint32_t* s_iters, float Wh, float Hh, float delta2, int lane, int wid,
                                                unsigned long long& box_evals) {
  for (int w = threadIdx.x; w < (n_tiles + 31) / 32; w += THREADS) s_dead[w] = s_dead0 ? s_dead0[w] : 0u;
  if (threadIdx.x == 0) s_cnt[0] = 0u;   // "a tile of this workgroup is still alive" (s_cnt is free until the epilogue)
  const float lim_box = 0.5f * (1.f + kTieEps) * __uint_as_float(gb_bits);
  // (tiles the group's common pre-pass has rejected are not looked at again)
  // Round 6: behind a VALID common mask (k6_group_prepass, state 1) the workgroup walks what the mask leaves, without a pre-pass of
  // its own -- the compaction rounds, three barriers and ~60 evaluations per live tile bought little once the common pre-pass
  // looked at twice the sample: full pass alone 0.323 -> 0.308 ms per 1024 frames (executed evaluations 251 -> 261 M), bench
  // 1 247 -> 1 274 k frames/s, config 5 87.3 -> 89.2 k; with groups of 7 thetas instead of 5 (the common pre-pass is then the only
  // filter and costs less per theta): 1 280 k / 92 k (groups of 3 / 4 / 5 / 7 / 9 / 11 / 15: 1 235 / 1 250 / 1 276 / 1 280 / 1 283 /
  // 1 271 / 1 177 k and 82.9 / 83.9 / 89.7 / 91.5 / 92.6 / 92.2 / 90.8 k).  Grids without a common pre-pass (state 2) keep their own.
  uint32_t wave_evals = 0;
  if (s_dead0 != nullptr) {
    if (threadIdx.x == 0) s_cnt[0] = 1u;   // (the group's state word said: some tile is alive)
  } else {
    wave_evals = box_prepass_rounds<THREADS>(n_tiles, ntb, a_org, b_org, n_ty, n_tz, s_ay, s_az, s_dead, s_live, s_cnt + 1, s_cnt, n_pre,
                                             lim_box, Wh, Hh, delta2, [&](uint32_t u) {
                                               const float2 v = s_ij[Mi + u];
                                               return make_float4(v.x, v.x, v.y, v.y);
                                             });
  }
  if (lane == 0) s_iters[wid] = wave_evals;   // (s_iters is free until the epilogue)
  __syncthreads();
  for (int w = 0; w < THREADS / ILCC_WAVE; ++w) box_evals += s_iters[w];
  const bool any_alive = s_cnt[0] != 0u;
  __syncthreads();
  return any_alive;
}

// The workgroup's record: the argmin over its wavefronts' bests, with (a << 16) | b of the winner, and its executed work
template <int THREADS>
__device__ __forceinline__ void publish_record(const Ctx& c, uint32_t f, Best best, uint32_t pts_done, uint32_t pts_in, bool use_box, unsigned long long box_evals,
                                               int n_ty, int n_tz, Best* s_best, uint32_t* s_iters, uint32_t* s_cnt, int lane, int wid, GridPartial* out) {
  // lanes hold different candidates: wavefront argmin, then across the 4 wavefronts
  best = wave_argmin(best);
  if (lane == 0) {
    s_best[wid] = best;
    s_iters[wid] = pts_done;
    s_cnt[wid] = pts_in;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t it_sum = 0, in_sum = 0;
    for (int w = 0; w < THREADS / ILCC_WAVE; ++w) {
      it_sum += s_iters[w];
      in_sum += s_cnt[w];
    }
    count_evals(c.grid_iters, f, kEvalsAll, it_sum);
    count_evals(c.grid_iters, f, kEvalsInterior, in_sum);
    if (use_box) count_evals(c.grid_iters, f, kEvalsBox, box_evals);
    uint32_t none = 0;
    const Best b = block_argmin<THREADS / ILCC_WAVE>(s_best, nullptr, none);
    out->cost = b.cost;
    out->d2 = b.d2;
    out->flat = b.flat;
    // (a << 16) | b of the winner in this launch's tables: the next launch reads it instead of dividing the flat index
    uint32_t ab = 0;
    if (b.flat != 0xFFFFFFFFu) {
      const uint32_t cell = b.flat >> 1;
      ab = (((cell / (uint32_t)n_tz) % (uint32_t)n_ty) << 16) | (cell % (uint32_t)n_tz);
    }
    out->pad = ab;
  }
}

// OVERFLOW (round 6; LDS_POINTS only): the frame holds more labelled points than the workgroup's LDS staging (Ctx::grid_lds_points:
// the handle stops growing it where a second workgroup would no longer fit the CU).  The first grid_lds_points walk positions are
// staged as always -- the box pre-pass's sample and the blocks nearly every tile dies on are among them --, a position past them is
// read from the walk layout in L2 and rotated by the lane that needs it: only the few tiles that walk (almost) the whole frame get
// there.  Same points, same order, same sums.  (Before: such a frame took the LDS-free body, which has no box pre-pass: a handful of
// frames with 6 682 labelled points made config 5's full pass 5.6 ms instead of 0.74 ms per 128 frames.)
// OVERFLOW = 2 (staged_prefix = false): the interior class and the box pre-pass's sample do not fit the staging, so NOTHING is staged
// and there is no box pre-pass -- every position comes from the walk layout in L2 -- but the walk, and with it every candidate's fp32
// sum, stays the staged form's.  (Such a frame used to take the LDS-free body, which adds the points in another order: its grid
// cost, and on a near tie the fp32 ranking, then depended on the handle's capacity.)
// (A template value, not a run-time flag: with the flag the pipeline's kernels compiled to another schedule.)
template <bool OOB, bool VOLUME, bool LDS_POINTS, bool PRUNE, int THREADS, int OVERFLOW = 0>
__device__ __forceinline__ void grid_cost_body(const Ctx& c, const GridPass& pass, float* volume, float2* s_ij, float* s_hw, Best* s_best,
                                               uint32_t* s_iters, uint32_t* s_cnt, float* s_ay, float* s_az, uint32_t* s_dead, uint16_t* s_live,
                                               uint32_t* s_next, const uint32_t kblk, const uint32_t f) {
  constexpr bool staged_prefix = OVERFLOW != 2;
  // kblk: this workgroup's index within the frame, f: its frame (blockIdx.x, blockIdx.y of the (n_th, F) launch; from the item of the listed one)
  uint32_t k = kblk;   // theta index (a launch with a window: set from the seed below)
  [[maybe_unused]] const unsigned long long t_entry = K6_NOW();
  [[maybe_unused]] unsigned long long t_rej = 0, t_surv = 0, n_rej = 0, n_surv = 0, n_done = 0, p_surv = 0;
  [[maybe_unused]] unsigned long long n_tests = 0, alive_sum = 0, alive_le4 = 0, alive_le2 = 0;   // bound tests after the first one
  const ilcc_result* r = &c.res[f];
  const int lane = lane_id();
  const int wid = __builtin_amdgcn_readfirstlane(wave_id());
  constexpr int kBoxShift = kBoxShiftOf<THREADS>;
  GridPartial* out = &pass.out[(uint64_t)f * pass.blocks + kblk];
  // full pass behind k6_group_prepass: tiles the pre-pass common to this theta's group has already rejected (a bit mask in
  // global memory), or nothing at all to do when it rejected them all
  const uint32_t* s_dead0 = nullptr;
  bool group_dead = false;
  if constexpr (PRUNE && OOB && LDS_POINTS && !VOLUME) {
    if (pass.grp_alive != nullptr) {
      const uint32_t tr = (uint32_t)f * pass.grp_count + kblk / (uint32_t)kThetaGroup;
      const uint32_t st = pass.grp_alive[tr];   // 0: every tile dead, 1: mask valid, 2: no common pre-pass ran for this group
      group_dead = st == 0u;
      if (st == 1u) s_dead0 = pass.grp_mask + (uint64_t)tr * pass.grp_words;
    }
  }
  if (r->status != ILCC_OK || group_dead) {
    if (threadIdx.x == 0) no_candidate(out);
    return;
  }
  // walk_limit: the seed and refinement launches only look at a PREFIX of the walk -- the golden-ratio order makes it a
  // uniform sample of the board -- to find WHERE the minimum is; their sums are not costs of complete candidates and go to
  // a bound word of their own.  The anchor launch then evaluates the found neighbourhood on every point: that is the bound.
  // (the LDS-free body walks the frame's own arrays in golden-ratio order, layout or not)
  const uint32_t Mfull = c.n_lab[f];
  const uint32_t M = pass.walk_limit ? walk_sample(Mfull, pass.walk_limit) : Mfull;   // an eighth of the points (measured: 1/2: 323 k, 1/4: 331 k, 1/8: 335 k, 1/16: 329 k frames/s), at least walk_limit
  const uint64_t beg = c.off[f];
  const float2* __restrict__ gyz = c.yz + beg;
  const uint8_t* __restrict__ glab = c.lab + beg;
  const int n_ty = pass.t.n_ty, n_tz = pass.t.n_tz;
  int nta = axis_tiles(n_ty), ntb = axis_tiles(n_tz);
  int a_org = 0, b_org = 0;   // first candidate of tile (0, 0)
  int t0 = 0;
  if (PRUNE && pass.seed.records != nullptr) {
    uint32_t k2u, ab;
    const Best sb = seed_argmin(pass.seed, f, k2u, ab);
    if (sb.flat != 0xFFFFFFFFu) {
      const int a2 = __builtin_amdgcn_readfirstlane((int)(ab >> 16)), b2 = __builtin_amdgcn_readfirstlane((int)(ab & 0xFFFFu));
      const int k2 = __builtin_amdgcn_readfirstlane((int)k2u);
      const int sa = min(a2 * pass.seed.map.stride_t, n_ty - 1), sbb = min(b2 * pass.seed.map.stride_t, n_tz - 1);
      if (pass.window_tiles) {
        // refinement pass: every candidate within +-radius theta steps and the 8 x 8 (ty, tz) window
        // around the seed argmin -> the frame's bound is (nearly always) the true minimum before the
        // full pass starts, which is what lets the full pass cut almost every tile after 8 points
        // (it scores every kRefineThetaStride-th theta of its range: step_th; the anchor rounds -- k6_anchor, or the tail of k6_locate -- cover the ones in between)
        const int kc = pass.seed.map.off_th + k2 * pass.seed.map.stride_th + (int)kblk * pass.step_th - pass.radius_th;
        k = (uint32_t)__builtin_amdgcn_readfirstlane(min(max(kc, 0), pass.t.n_th - 1));
        // window_tiles = tiles per axis of the window: 2 (8 x 8 translations around the seed's argmin) or, on grids whose seed stride
        // is wider than that window (config 5: every 16th translation), 4 -- the seed's best can be half a stride from the minimum
        const int wt = max(2, pass.window_tiles);
        a_org = __builtin_amdgcn_readfirstlane(window_origin(sa, (wt * kTile) / 2, n_ty, wt * kTile));
        b_org = __builtin_amdgcn_readfirstlane(window_origin(sbb, (wt * kTile) / 2, n_tz, wt * kTile));
        nta = min(wt, nta);
        ntb = min(wt, ntb);
      } else {
        // full pass: start at the tile that holds the seed's best translation; the order never changes the result
        t0 = __builtin_amdgcn_readfirstlane((sa / kTile) * ntb + (sbb / kTile));
      }
    }
  }
  const float cth = pass.t.cth[k], sth = pass.t.sth[k];

  // Point order: k5w_walk_order (k5w_walk_order.hip) has written the frame's labelled points in WALK layout (FrameWalk), once per frame instead
  // of once per workgroup.  Golden-ratio order makes every prefix of a part a sample spread over the whole board: the bound test
  // cuts tiles sooner than ring order would.  INTERIOR: in the board under EVERY rotation and translation of the tables ->
  // accumulate_interior.  Staging is then a rotation of M points by this workgroup's theta.  A subsampled launch (walk_limit)
  // stages a prefix of each part, in proportion.
  uint32_t Mi = 0;
  uint32_t stage_lo = 0, stage_hi = 0;   // walk positions staged so far: [stage_lo, stage_hi)
  const uint32_t S = Mfull ? c.walk_stride[f] : 1u;
  const float2* __restrict__ wyz = c.walk_yz + beg;
  const uint8_t* __restrict__ wlab = c.walk_lab + beg;
  const uint32_t Mi_all = LDS_POINTS ? c.walk_mi[f] : 0u, n_rim_all = LDS_POINTS ? c.walk_nrim[f] : 0u;
  uint32_t n_in, n_rm;
  walk_prefix(M, Mfull, Mi_all, n_rim_all, n_in, n_rm);
  auto walk_source = [&](uint32_t sl) { return layout_source(sl, n_in, n_rm, Mfull, Mi_all, n_rim_all); };
  const uint32_t lds_n = OVERFLOW ? (staged_prefix ? min(M, c.grid_lds_points) : 0u) : M;   // walk positions [0, lds_n) live in LDS
  auto stage_point = [&](uint32_t sl) {
    const uint32_t src = walk_source(sl);
    s_ij[sl] = rotate(wyz[src], cth, sth);
    s_hw[sl] = wlab[src] ? 0.5f : 0.f;
  };
  if (LDS_POINTS) {
    Mi = n_in;
    // The full pass stages the points its box pre-pass looks at first: a workgroup the pre-pass leaves no tile (half of
    // them: every theta more than a few steps from the minimum) never stages, or reads, the rest.
    const bool box_first = PRUNE && OOB && pass.box_points != 0u && nta * ntb <= kBoxTilesMax && M > Mi && (!OVERFLOW || staged_prefix);   // (= use_box below)
    stage_lo = box_first ? Mi : 0u;
    stage_hi = box_first ? Mi + box_sample(pass.box_points, Mfull, M, Mi, kBoxShift) : lds_n;   // (OVERFLOW: the caller made sure the sample fits)
    for (uint32_t sl = stage_lo + threadIdx.x; sl < stage_hi; sl += THREADS) stage_point(sl);
  }
  // (ty, tz) tables in LDS: a cut-short tile lasts about as long as one L2 round trip, so its
  // prologue must not wait for global loads
  for (int i = threadIdx.x; i < n_ty; i += THREADS) s_ay[i] = pass.t.ay[i];
  for (int i = threadIdx.x; i < n_tz; i += THREADS) s_az[i] = pass.t.az[i];
  if (threadIdx.x == 0) *s_next = 0u;   // the workgroup's tile-chunk counter (see the tile loop)
  __syncthreads();
  [[maybe_unused]] const unsigned long long t_staged = K6_NOW();

  const float Wh = 0.5f * (float)c.p.board_w, Hh = 0.5f * (float)c.p.board_h;
  const float delta2 = (float)c.p.huber_delta;   // (the terms carry plain r and q: a lane's sums are cost / 2)
  const int n_tiles = nta * ntb;
  const uint32_t dk = (uint32_t)((int)k - pass.t.c_th) * (uint32_t)((int)k - pass.t.c_th);

  Best best{__builtin_inff(), 0xFFFFFFFFu, 0xFFFFFFFFu};
  uint32_t* bound = pass.bound + f;
  float shared_bound = __builtin_inff();   // what this wavefront last published
  uint32_t gb_bits = PRUNE ? __hip_atomic_load(bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0x7f800000u;
  uint32_t pts_done = 0, pts_in = 0;   // walk positions executed by this wavefront (all / interior class)

  // BOX PRE-PASS (full pass of the pipeline): a lower bound for all 16 candidates of a tile at once, at the price of ONE
  // evaluation per point.  A border-class point that is out of the board under EVERY translation of the tile's 4 x 4 box costs
  // each of them at least T(r_box), r_box = (smallest |u_i| over the box) + (smallest |u_j| over the box): u = |x - W/2| - W/2
  // is evaluated with accumulate<>'s own fp32 expressions at the two extreme translations of each axis, every operation in
  // it is monotone (floating-point rounding included) and a box is narrower than one square (the host checks), so the
  // extremes bound everything in between; T is non-decreasing in r, and both colour phases pay an out-of-board point.  Points
  // that are in the board somewhere in the box count 0.  lane = (tile, half of the points): 2 x box_points evaluations per
  // tile instead of the 16 x 8 of a first block -- and the rim points, which the walk puts first, are exactly the ones that
  // leave the board when the translation is wrong.  A tile whose bound already exceeds the frame's bound is never started.
  // kBoxSafety: the bound is a sum in another order than the candidates' own fp32 sums (<= 2^12 terms per lane).
  bool use_box = false;
  unsigned long long box_evals = 0;   // (point, tile) evaluations of this workgroup's pre-pass
  if constexpr (PRUNE && LDS_POINTS && OOB) {
    use_box = pass.box_points != 0u && n_tiles <= kBoxTilesMax && M > Mi && (!OVERFLOW || staged_prefix);
    if (use_box) {
      const uint32_t n_pre = box_sample(pass.box_points, Mfull, M, Mi, kBoxShift);
      const bool any_alive = own_box_prepass<THREADS>(n_tiles, ntb, a_org, b_org, n_ty, n_tz, s_ay, s_az, s_ij, Mi, n_pre, gb_bits, s_dead0, s_dead, s_live, s_cnt,
                                                      s_iters, Wh, Hh, delta2, lane, wid, box_evals);
      if (!any_alive) {   // nothing to walk at this theta: the rest of the frame's points is never staged
        if (threadIdx.x == 0) {
          no_candidate(out);
          count_evals(c.grid_iters, f, kEvalsBox, box_evals);
        }
        return;
      }
      for (uint32_t sl = threadIdx.x; sl < stage_lo; sl += THREADS) stage_point(sl);
      for (uint32_t sl = stage_hi + threadIdx.x; sl < lds_n; sl += THREADS) stage_point(sl);
      __syncthreads();
    }
  }
  float* vol = VOLUME ? volume + (uint64_t)f * (uint64_t)pass.t.n_th * n_ty * n_tz * 2u : nullptr;
  const int my_s = lane & (kSlices - 1), my_c = lane >> 2;
  const int my_a = my_c >> 2, my_b = my_c & 3;

  // first block of each class in registers (see run_tile); needs a full block of both classes
  constexpr int kFirstIn = 0, kFirstBd = 2;   // interior- / border-class (rim-first) points per lane in the first, register-resident block
  const bool first_block = LDS_POINTS && Mi >= (uint32_t)(kFirstIn * kSlices) && M - Mi >= (uint32_t)(kFirstBd * kSlices);
  PointTerms first_in[kFirstIn > 0 ? kFirstIn : 1], first_bd[kFirstBd > 0 ? kFirstBd : 1];
  auto first_point = [&](uint32_t at) -> PointTerms {
    if (OVERFLOW == 2 && at >= lds_n) {   // (nothing is staged)
      const uint32_t src = walk_source(at);
      const float2 v = rotate(wyz[src], cth, sth);
      return PointTerms{v.x, v.y, wlab[src] ? 0.5f : 0.f};
    }
    const float2 v = s_ij[at];
    return PointTerms{v.x, v.y, s_hw[at]};
  };
  if (LDS_POINTS && first_block) {
#pragma unroll
    for (int u = 0; u < kFirstIn; ++u) first_in[u] = first_point((uint32_t)(u * kSlices + my_s));
#pragma unroll
    for (int u = 0; u < kFirstBd; ++u) first_bd[u] = first_point(Mi + (uint32_t)(u * kSlices + my_s));
  }

  const bool whole_tiles = (n_ty % kTile) == 0 && (n_tz % kTile) == 0;   // (wave-uniform: a scalar branch per tile)
  // one 4 x 4 tile, quad-sliced (lane = candidate * 4 + slice), from walk positions (pin0, pbd0) on, sums starting at
  // (a0_init, a1_init)
  auto run_tile = [&](int tile_a, int tile_b, float a0_init, float a1_init, uint32_t pin0, uint32_t pbd0) {
    const int ia = a_org + tile_a * kTile + my_a, ib = b_org + tile_b * kTile + my_b;
    // grids whose axes are multiples of the tile (the default 40 x 40) have no partial tiles: no clamps, no owner test
    bool owner = true;
    unsigned long long owner_mask = ~0ull;   // an SGPR pair: the bound test is then ballot & mask, no VALU select
    float ay, az;
    if (whole_tiles) {
      ay = s_ay[ia];
      az = s_az[ib];
    } else {
      owner = ia < n_ty && ib < n_tz;
      owner_mask = __ballot(owner);
      ay = s_ay[min(ia, n_ty - 1)];
      az = s_az[min(ib, n_tz - 1)];
    }

    // Branch and bound (PRUNE): costs are sums of non-negative terms, so a candidate whose partial
    // sum already exceeds the best COMPLETE cost known for this frame cannot be the argmin.
    // Exact: only provably losing candidates are cut short.
    float A0 = a0_init, A1 = a1_init;
    bool pruned = false;
    // the shared bound is fetched ahead of its use (an L2 round trip is longer than a cut-short tile, and a
    // slightly stale bound only delays a cut): this tile starts with the word loaded during the previous
    // one and issues the load for the next refresh right away
    // sums are cost / 2.  The test keeps everything within kTieEps of the bound alive: fp32 sums cannot order
    // such candidates reliably, K7r re-orders them on exact fixed-point sums
    float lim2 = 0.5f * (1.f + kTieEps) * fminf(__uint_as_float(gb_bits), best.cost);
    if (PRUNE) gb_bits = __hip_atomic_load(bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // lane's points: walk positions my_s, my_s + 4, ...  (LDS_POINTS = false: point index (pos * S) mod M)
    // (M == 0: no point is ever fetched, every candidate costs 0; keep the modulo defined)
    uint32_t idx = Mfull ? (uint32_t)(((uint64_t)my_s * S) % Mfull) : 0u;
    const uint32_t idx_step = Mfull ? (uint32_t)(((uint64_t)kSlices * S) % Mfull) : 0u;
    uint32_t pos = 0;
    auto fetch = [&](uint32_t at) -> PointTerms {   // at = walk position of THIS lane's point
      if (LDS_POINTS) {
        if (OVERFLOW && at >= lds_n) {   // past the staged prefix: from the walk layout in L2, rotated here
          const uint32_t src = walk_source(at);
          const float2 v = rotate(wyz[src], cth, sth);
          return PointTerms{v.x, v.y, wlab[src] ? 0.5f : 0.f};
        }
        const float2 v = s_ij[at];
        return PointTerms{v.x, v.y, s_hw[at]};
      } else {
        const float2 v = rotate(gyz[idx], cth, sth);
        const PointTerms t{v.x, v.y, glab[idx] ? 0.5f : 0.f};
        idx += idx_step;
        if (idx >= Mfull) idx -= Mfull;
        return t;
      }
    };
    [[maybe_unused]] uint32_t pin = pin0, pbd = pbd0;   // next walk position of each class (the staged walk)
    auto beaten = [&]() -> bool {          // every candidate of the tile provably loses
      const float part = fminf(quad_sum(A0), quad_sum(A1));
#ifdef ILCC_K6_TIMING
      {
        const uint32_t alive = (uint32_t)__popcll(__ballot(!(part > lim2)) & owner_mask) >> 2;
        if (pin + (pbd - Mi) > (uint32_t)((kFirstIn + kFirstBd) * kSlices) && alive) {
          ++n_tests;
          alive_sum += alive;
          alive_le4 += alive <= 4u;
          alive_le2 += alive <= 2u;
        }
      }
#endif
      return (__ballot(!(part > lim2)) & owner_mask) == 0ull;
    };
    if constexpr (LDS_POINTS) {
      // Two interleaved walks: 8 interior points (cheap term), 8 border points (full term), test, ... --
      // interleaved so that every prefix still samples both the pattern (interior) and the outline (border) of the board
      uint32_t since_refresh = 0;
      auto refresh = [&]() {
        since_refresh += kStep;
        if (since_refresh >= (uint32_t)kBoundRefresh) {
          since_refresh = 0;
          lim2 = 0.5f * (1.f + kTieEps) * fminf(__uint_as_float(gb_bits), best.cost);
          gb_bits = __hip_atomic_load(bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next refresh
        }
      };
      // The first block of each class is the SAME 16 walk positions for every tile of the workgroup, and 96 % of the tiles
      // die at the test that follows it: those points live in registers (first_in / first_bd, loaded once per wavefront), so
      // the rejection path of a tile touches LDS only for its (ty, tz) pair and never prefetches a block it will not use
      if (first_block) {
#pragma unroll
        for (int u = 0; u < kFirstIn; ++u) accumulate_interior(first_in[u], ay, az, delta2, A0, A1);
#pragma unroll
        for (int u = 0; u < kFirstBd; ++u) accumulate<OOB>(first_bd[u], ay, az, Wh, Hh, delta2, A0, A1);
        pin = kFirstIn * kSlices;
        pbd = Mi + kFirstBd * kSlices;
        if (PRUNE) {
          if (beaten())
            pruned = true;
          else
            refresh();
        }
      }
      // Survivors of the first test -- 72 % of the kernel's VALU instructions are spent here (tools/dev_k6_timing.py) -- walk
      // on in a loop made for the common case, "both classes still have a full block": one bound test per 8 + 8 positions, a
      // scalar trip count, and NO software prefetch: with 6-7 resident wavefronts per SIMD the LDS latency is covered by the
      // other wavefronts, and the registers of a second block in flight cost a wavefront of occupancy (measured with two
      // named register sets: 83 VGPRs, 267 k instead of 281 k frames/s).
      if (!(PRUNE && pruned)) {
        constexpr int kLoopIn = 0, kLoopBd = 3;   // interior- / border-class points per lane and trip of this loop
        constexpr uint32_t kStepIn = kLoopIn * kSlices, kStepBd = kLoopBd * kSlices;
        uint32_t both = (uint32_t)__builtin_amdgcn_readfirstlane(
            (int)min(kLoopIn ? (Mi - min(pin, Mi)) / (kLoopIn ? kStepIn : 1u) : 0x7FFFFFFFu, kLoopBd ? (M - pbd) / (kLoopBd ? kStepBd : 1u) : 0x7FFFFFFFu));
        for (; both; --both) {
          PointTerms bi[kLoopIn > 0 ? kLoopIn : 1], bb[kLoopBd > 0 ? kLoopBd : 1];
#pragma unroll
          for (int u = 0; u < kLoopIn; ++u) bi[u] = fetch(pin + u * kSlices + my_s);
#pragma unroll
          for (int u = 0; u < kLoopBd; ++u) bb[u] = fetch(pbd + u * kSlices + my_s);
#pragma unroll
          for (int u = 0; u < kLoopIn; ++u) accumulate_interior(bi[u], ay, az, delta2, A0, A1);
#pragma unroll
          for (int u = 0; u < kLoopBd; ++u) accumulate<OOB>(bb[u], ay, az, Wh, Hh, delta2, A0, A1);
          pin += kStepIn;
          pbd += kStepBd;
          since_refresh += kStepIn + kStepBd - kStep;   // (refresh() adds kStep)
          if (PRUNE) {
            if (beaten()) {
              pruned = true;
              break;
            }
            refresh();
          }
        }
      }
      // what is left when one class runs out of full blocks (a few dozen positions at the end of a complete walk)
      for (; !(PRUNE && pruned);) {
        const bool more_in = pin + kStep <= Mi, more_bd = pbd + kStep <= M;
        if (!more_in && !more_bd) break;
        if (more_in) {
#pragma unroll
          for (int u = 0; u < kUnroll; ++u) accumulate_interior(fetch(pin + u * kSlices + my_s), ay, az, delta2, A0, A1);
          pin += kStep;
        }
        if (more_bd) {
#pragma unroll
          for (int u = 0; u < kUnroll; ++u) accumulate<OOB>(fetch(pbd + u * kSlices + my_s), ay, az, Wh, Hh, delta2, A0, A1);
          pbd += kStep;
        }
        if (PRUNE) {
          if (beaten()) {
            pruned = true;
            break;
          }
          refresh();
        }
      }
      if (!(PRUNE && pruned)) {   // tails (< 8 points per class): one point per lane and trip, lanes past the end idle
        for (; pin < Mi; pin += kSlices) {
          const uint32_t at = pin + my_s;
          if (at < Mi) accumulate_interior(fetch(at), ay, az, delta2, A0, A1);
        }
        for (; pbd < M; pbd += kSlices) {
          const uint32_t at = pbd + my_s;
          if (at < M) accumulate<OOB>(fetch(at), ay, az, Wh, Hh, delta2, A0, A1);
        }
        pos = M;
        pts_in += Mi;
      } else {
        pos = pin + (pbd - Mi);
        pts_in += pin;
      }
    } else {
      PointTerms nxt[kUnroll];   // the next block's points are in flight while this block is evaluated
      if (kStep <= M) {
  #pragma unroll
        for (int u = 0; u < kUnroll; ++u) nxt[u] = fetch(u * kSlices + my_s);
      }
      for (; pos + kStep <= M; pos += kStep) {
        PointTerms pt[kUnroll];
  #pragma unroll
        for (int u = 0; u < kUnroll; ++u) pt[u] = nxt[u];
        if (pos + 2 * kStep <= M) {
  #pragma unroll
          for (int u = 0; u < kUnroll; ++u) nxt[u] = fetch(pos + kStep + u * kSlices + my_s);
        }
  #pragma unroll
        for (int u = 0; u < kUnroll; ++u) accumulate<OOB>(pt[u], ay, az, Wh, Hh, delta2, A0, A1);
        if (PRUNE) {
          if (beaten()) {
            pruned = true;
            pos += kStep;
            break;
          }
          if (((pos + kStep) & (kBoundRefresh - 1)) == 0) {   // (not refresh(): its counter compiles to another loop)
            lim2 = 0.5f * (1.f + kTieEps) * fminf(__uint_as_float(gb_bits), best.cost);
            gb_bits = __hip_atomic_load(bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next refresh
          }
        }
      }
      if (!(PRUNE && pruned)) {
        if (!LDS_POINTS && Mfull) idx = (uint32_t)(((uint64_t)(pos + my_s) * S) % Mfull);
        for (; pos < M; pos += kSlices) {   // tail (< 12 points): one point per lane and trip, lanes past the end idle
          const uint32_t at = pos + my_s;
          if (at < M) {
            const PointTerms p1 = fetch(at);
            accumulate<OOB>(p1, ay, az, Wh, Hh, delta2, A0, A1);
          }
        }
        pos = M;
      }
    }
    pts_done += pos;
    if (PRUNE && pruned) return;

    const float t0s = quad_sum(A0), t1s = quad_sum(A1);   // the four slices of each candidate
    if (owner) {
      const uint32_t cell = ((uint32_t)k * (uint32_t)n_ty + (uint32_t)ia) * (uint32_t)n_tz + (uint32_t)ib;
      const uint32_t d2 = dk + (uint32_t)((ia - pass.t.c_ty) * (ia - pass.t.c_ty)) + (uint32_t)((ib - pass.t.c_tz) * (ib - pass.t.c_tz));
      const float c0 = 2.f * t0s, c1 = 2.f * t1s;
      if (pass.collect_ties && my_s == 0 && fminf(c0, c1) <= 2.f * lim2) {   // full pass: near ties of the bound
        // completions are rare: afford a fresh look at the frame's bound so that little junk is listed while it is loose
        const float fresh = __uint_as_float(__hip_atomic_load(bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const float thr = (1.f + kTieEps) * fminf(fresh, fminf(best.cost, fminf(c0, c1)));
        // more than kTieCap entries: the count keeps growing, the consumer sees the overflow and falls back to the
        // (deterministic) fp32 argmin with ILCC_FLAG_TIE_OVERFLOW set -- which entries made it into the list never matters
        if (c0 <= thr) {
          const uint32_t at = atomicAdd(c.tie_count + f, 1u);
          if (at < (uint32_t)kTieCap) c.tie_list[(uint64_t)f * kTieCap + at] = GridPartial{c0, d2, 2u * cell, 0u};
        }
        if (c1 <= thr) {
          const uint32_t at = atomicAdd(c.tie_count + f, 1u);
          if (at < (uint32_t)kTieCap) c.tie_list[(uint64_t)f * kTieCap + at] = GridPartial{c1, d2, 2u * cell + 1u, 0u};
        }
      }
      if (better(c0, d2, 2u * cell, best)) best = Best{c0, d2, 2u * cell};
      if (better(c1, d2, 2u * cell + 1u, best)) best = Best{c1, d2, 2u * cell + 1u};
      if (VOLUME && my_s == 0) {
        vol[2u * cell] = c0;
        vol[2u * cell + 1u] = c1;
      }
    }
    if (PRUNE) {
      // share the wavefront's best complete cost with every workgroup of the frame
      const float wb = wave_min(best.cost);
      // publish only what improves the frame's bound as this wavefront last saw it: atomics on a
      // word that thousands of wavefronts also load serialise in L2 (measured: 2.5x on the kernel)
      if (lane == 0 && wb < fminf(shared_bound, __uint_as_float(gb_bits))) {
        shared_bound = wb;
        atomicMin(bound, __float_as_uint(wb));   // costs are >= 0: uint order == float order
      }
    }
  };

  // (Measured and rejected: a PRE-PASS that evaluates the first 8 + 8 walk positions with lane = candidate for four tiles
  // at once -- one LDS broadcast per point, no quad reduction, one prologue and one bound test per four tiles -- and lets
  // only the surviving tiles into the quad-sliced loop.  An instruction-count model from simulated death times promised
  // -12 %; on the chip: 85 instead of 72 VGPRs (5 instead of 7 waves per SIMD) and sixteen serial evaluations per lane:
  // 0.611 instead of 0.564 ms per batch, 235 k instead of 250.6 k frames/s.)
  // This wavefront's tiles are wid, wid + 4, ... of the order rotated by t0 (the tile of the seed's best translation first).
  // 64 of them at a time, one per lane: the lanes look their tiles up in the pre-pass's bit mask, a ballot gives the ones
  // still alive, and only those are visited (a handful of a wavefront's 25: the loop over dead tiles was a third of the
  // kernel's scalar instructions).
  const int ntb_s = __builtin_amdgcn_readfirstlane(ntb);
  auto visit = [&](int qs) {   // tile qs of the workgroup
    const int tile_a = __builtin_amdgcn_readfirstlane(qs / ntb_s), tile_b = __builtin_amdgcn_readfirstlane(qs - tile_a * ntb_s);
#ifdef ILCC_K6_TIMING
    const unsigned long long tt0 = K6_NOW();
    const uint32_t pd0 = pts_done;
#endif
    run_tile(tile_a, tile_b, 0.f, 0.f, 0u, Mi);
#ifdef ILCC_K6_TIMING
    const unsigned long long dt = K6_NOW() - tt0;
    const uint32_t walked = pts_done - pd0;
    if (walked <= (uint32_t)(2 * kStep) && walked < M) {
      ++n_rej;
      t_rej += dt;
    } else {
      ++n_surv;
      t_surv += dt;
      p_surv += walked;
      if (walked >= M) ++n_done;
    }
#endif
  };
  if constexpr (kIsLargeInstance<THREADS>) {
    // The 512-thread instance (frames of several thousand labelled points, ~1000 tiles per workgroup): which wavefront takes
    // which tile is decided at run time.  The tiles that survive the pre-pass AND walk far (the candidates around the minimum)
    // used to fall to whichever wavefront the static interleave gave them, and the workgroup waited at its last barrier for the
    // unlucky one (16 % of a wavefront's life on BASELINE config 5, tools/dev_k6_timing.py): 23.2 -> 24.0 k frames/s there.  (The
    // 256-thread instance keeps the static interleave below: with 100 tiles and 2.4 survivors per wavefront the claims cost
    // more than they balance -- 775 -> 740 k frames/s.)  A wavefront
    // claims CHUNKS of kChunk tile slots from a counter in LDS; slot n of chunk c is tile (c + n_chunks * n + t0) mod n_tiles,
    // so neighbouring tiles -- the expensive ones are neighbours -- sit in different chunks, and chunk 0 starts with the tile of
    // the seed's best translation.  The lanes look their slots up in the pre-pass's bit mask, a ballot gives the ones still
    // alive, and only those are visited.  The order never changes the result.
    constexpr int kChunk = 8;   // tile slots per claim
    static_assert(kChunk >= 1 && kChunk <= ILCC_WAVE, "a chunk is looked up by the lanes of one wavefront");
    const int n_chunks = __builtin_amdgcn_readfirstlane((n_tiles + kChunk - 1) / kChunk);
    for (;;) {
      int cl = 0;
      if (lane == 0) cl = (int)atomicAdd(s_next, 1u);
      const int ch = __builtin_amdgcn_readfirstlane(cl);
      if (ch >= n_chunks) break;
      bool alive = false;
      if (lane < kChunk) {
        const int slot = ch + n_chunks * lane;
        if (slot < n_tiles) {
          int q = slot + t0;
          if (q >= n_tiles) q -= n_tiles;
          alive = !use_box || !((s_dead[q >> 5] >> (q & 31)) & 1u);
        }
      }
      unsigned long long todo = __ballot(alive);
      while (todo) {
        const int bit = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(todo));
        todo &= todo - 1ull;
        int qs = ch + n_chunks * bit + t0;
        if (qs >= n_tiles) qs -= n_tiles;
        visit(qs);
      }
    }
  } else {
    constexpr int kWaves = THREADS / ILCC_WAVE;
    const int per_wave = __builtin_amdgcn_readfirstlane(wid < n_tiles ? (n_tiles - wid + kWaves - 1) / kWaves : 0);
    for (int k0 = 0; k0 < per_wave; k0 += ILCC_WAVE) {
      bool alive = false;
      if (k0 + lane < per_wave) {
        int q = wid + kWaves * (k0 + lane) + t0;
        if (q >= n_tiles) q -= n_tiles;
        alive = !use_box || !((s_dead[q >> 5] >> (q & 31)) & 1u);
      }
      unsigned long long todo = __ballot(alive);
      while (todo) {
        const int bit = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(todo));
        todo &= todo - 1ull;
        int qs = wid + kWaves * (k0 + bit) + t0;
        if (qs >= n_tiles) qs -= n_tiles;
        visit(qs);
      }
    }
  }
  [[maybe_unused]] const unsigned long long t_tiles = K6_NOW();

  publish_record<THREADS>(c, f, best, pts_done, pts_in, use_box, box_evals, n_ty, n_tz, s_best, s_iters, s_cnt, lane, wid, out);
#ifdef ILCC_K6_TIMING
  if (lane == 0 && pass.collect_ties) {   // the full pass only
    const unsigned long long t_end = K6_NOW();
    const uint32_t w = ((f * pass.blocks + kblk) * (THREADS / ILCC_WAVE) + (uint32_t)wid) & (kProfWaves - 1);
    unsigned long long* o = k6_prof + (size_t)w * kProfWords;
    o[0] = 1ull;
    o[1] = t_end - t_entry;
    o[2] = t_staged - t_entry;
    o[3] = n_rej;
    o[4] = t_rej;
    o[5] = n_surv;
    o[6] = t_surv;
    o[7] = p_surv;
    o[8] = n_done;
    o[9] = t_end - t_tiles;
    o[10] = (unsigned long long)M;
    o[11] = (unsigned long long)Mi;
    o[12] = n_tests;
    o[13] = alive_sum;
    o[14] = alive_le4;
    o[15] = alive_le2;
  }
#endif
}

// dynamic LDS: grid_lds (k6_common.h) for grid_lds_points staged points; frames with more labelled points than that read (and
// rotate) them through L1/L2 instead.
// THREADS: 256 (4 wavefronts) is the measured optimum for VLP-16-sized frames; frames of several thousand labelled points
// (BASELINE config 5: 4 198) stage 50+ KB per workgroup, three workgroups fit a CU, and 512 threads then double the
// resident wavefronts per SIMD (3 -> 6).  Same sums either way: a candidate's points are added by its quad in walk order.
template <bool OOB, bool VOLUME, bool PRUNE, int THREADS>
__global__ __launch_bounds__(THREADS) void k6_grid_cost(Ctx c, GridPass pass, float* volume) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ Best s_best[THREADS / ILCC_WAVE];
  __shared__ uint32_t s_iters[THREADS / ILCC_WAVE];
  __shared__ uint32_t s_cnt[THREADS / ILCC_WAVE];
  __shared__ uint32_t s_dead[kBoxTilesMax / 32];   // box pre-pass: one bit per tile of the workgroup
  __shared__ uint16_t s_live[kBoxSegment<THREADS>];         // box pre-pass: the tiles still alive, compacted
  __shared__ uint32_t s_next;                      // next chunk of tiles to hand to a wavefront
  const GridLds l = grid_lds(c.grid_lds_points, 0, 0);   // (the points' parts; the tables follow)
  float2* s_ij = reinterpret_cast<float2*>(smem);
  float* s_hw = lds_next<float>(smem, 0, l.hw);
  float* s_ay = lds_next<float>(s_hw, l.hw, l.ay);   // n_ty floats
  float* s_az = s_ay + pass.t.n_ty;                  // n_tz floats (taken from l.az: another kernarg load order in the two VOLUME instances)
  const uint32_t Mall = c.n_lab[blockIdx.y];
  // (unused, and kept on measurement: without it the full pass compiles to another schedule, same registers -- 6.2 k of the 10 k lines
  // of its gfx950 assembly differ -- and is slower: alone on the chip 0.350 against 0.342 ms per 1024 frames, five alternating
  // benchmark runs each 1 222 k against 1 241 k frames/s (medians; config 5: 96.9 against 96.3 k, inside its spread))
  const uint32_t M = pass.walk_limit ? walk_sample(Mall, pass.walk_limit) : Mall;
  (void)M;
  // (the choice of form below, and the LDS declared and carved above, have a COPY for the listed launch: listed_item and
  // K6_FULL_PASS_LDS further down -- a change here is a change there)
  if (Mall <= c.grid_lds_points) {   // (k5w_walk_order has laid out every frame of at most kGridLdsPointsMax points)
    grid_cost_body<OOB, VOLUME, true, PRUNE, THREADS>(c, pass, volume, s_ij, s_hw, s_best, s_iters, s_cnt, s_ay, s_az, s_dead, s_live, &s_next, blockIdx.x, blockIdx.y);
    return;
  }
  if constexpr (OOB && !VOLUME && PRUNE) {
    // the pipeline's full pass on a frame above the staging capacity: the staged prefix + the rest through L2, as long as the
    // interior class and the box pre-pass's sample (what every workgroup reads) are inside the prefix
    constexpr int kBoxShift = kBoxShiftOf<THREADS>;
    if (pass.walk_limit == 0u && pass.box_points != 0u && Mall <= (uint32_t)kGridLdsPointsMax) {
      const uint32_t Mi = c.walk_mi[blockIdx.y];
      // (= box_sample, written out: called here, the helper compiles both pipeline instances to another schedule, + 24 instructions)
      const bool staged_prefix = Mall > Mi && Mi + min(max(pass.box_points, Mall >> kBoxShift), Mall - Mi) <= c.grid_lds_points;
      if (staged_prefix)
        grid_cost_body<OOB, VOLUME, true, PRUNE, THREADS, 1>(c, pass, volume, s_ij, s_hw, s_best, s_iters, s_cnt, s_ay, s_az, s_dead, s_live, &s_next,
                                                             blockIdx.x, blockIdx.y);
      else
        grid_cost_body<OOB, VOLUME, true, PRUNE, THREADS, 2>(c, pass, volume, s_ij, s_hw, s_best, s_iters, s_cnt, s_ay, s_az, s_dead, s_live, &s_next,
                                                             blockIdx.x, blockIdx.y);
      return;
    }
  }
  grid_cost_body<OOB, VOLUME, false, PRUNE, THREADS>(c, pass, volume, s_ij, s_hw, s_best, s_iters, s_cnt, s_ay, s_az, s_dead, s_live, &s_next, blockIdx.x, blockIdx.y);
}

// ---- The full pass behind k6_group_prepass's hand-over (GridPass::work_list): only the listed (frame, theta) workgroups are started;
// the pre-pass has already written the records of all the others.  Same body, same sums, same records as the (n_th, F) launch.

// item `i` of the list: the form choice of k6_grid_cost above for the item's frame.  (A copy, not a shared helper: with the choice
// moved into a function of both kernels, the two pipeline instances of k6_grid_cost compile to another schedule -- 9.8 k of their
// 9.4 k lines of gfx950 assembly differ --, which this kernel is known not to take lightly: see (void)M above.)
template <int THREADS>
__device__ __forceinline__ void listed_item(const Ctx& c, const GridPass& pass, uint32_t i, float2* s_ij, float* s_hw, Best* s_best, uint32_t* s_iters,
                                            uint32_t* s_cnt, float* s_ay, float* s_az, uint32_t* s_dead, uint16_t* s_live, uint32_t* s_next) {
  const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)pass.work_list[i]);
  if (item >= c.n_frames * pass.blocks) return;   // (never: an item is the index of a record)
  const uint32_t f = item / pass.blocks, kblk = item - f * pass.blocks;
  const uint32_t Mall = c.n_lab[f];
  if (Mall <= c.grid_lds_points) {
    grid_cost_body<true, false, true, true, THREADS>(c, pass, nullptr, s_ij, s_hw, s_best, s_iters, s_cnt, s_ay, s_az, s_dead, s_live, s_next, kblk, f);
    return;
  }
  if (pass.walk_limit == 0u && pass.box_points != 0u && Mall <= (uint32_t)kGridLdsPointsMax) {   // OVERFLOW: the same conditions as in k6_grid_cost
    const uint32_t Mi = c.walk_mi[f];
    const bool staged_prefix = Mall > Mi && Mi + min(max(pass.box_points, Mall >> kBoxShiftOf<THREADS>), Mall - Mi) <= c.grid_lds_points;
    if (staged_prefix)
      grid_cost_body<true, false, true, true, THREADS, 1>(c, pass, nullptr, s_ij, s_hw, s_best, s_iters, s_cnt, s_ay, s_az, s_dead, s_live, s_next, kblk, f);
    else
      grid_cost_body<true, false, true, true, THREADS, 2>(c, pass, nullptr, s_ij, s_hw, s_best, s_iters, s_cnt, s_ay, s_az, s_dead, s_live, s_next, kblk, f);
    return;
  }
  grid_cost_body<true, false, false, true, THREADS>(c, pass, nullptr, s_ij, s_hw, s_best, s_iters, s_cnt, s_ay, s_az, s_dead, s_live, s_next, kblk, f);
}

// the LDS of a full-pass workgroup, as k6_grid_cost declares and carves it
#define K6_FULL_PASS_LDS(THREADS)                                                        \
  extern __shared__ __align__(16) unsigned char smem[];                                  \
  __shared__ Best s_best[THREADS / ILCC_WAVE];                                           \
  __shared__ uint32_t s_iters[THREADS / ILCC_WAVE];                                      \
  __shared__ uint32_t s_cnt[THREADS / ILCC_WAVE];                                        \
  __shared__ uint32_t s_dead[kBoxTilesMax / 32];                                         \
  __shared__ uint16_t s_live[kBoxSegment<THREADS>];                                      \
  __shared__ uint32_t s_next;                                                            \
  const GridLds l = grid_lds(c.grid_lds_points, 0, 0);                                   \
  float2* s_ij = reinterpret_cast<float2*>(smem);                                        \
  float* s_hw = lds_next<float>(smem, 0, l.hw);                                          \
  float* s_ay = lds_next<float>(s_hw, l.hw, l.ay);                                       \
  float* s_az = s_ay + pass.t.n_ty

// k6_grid_cost_listed: a 1-D grid of G workgroups, workgroup b runs item b -- straight-line code, the registers of the (n_th, F)
// launch (64 VGPRs, seven wavefronts per SIMD).  G is the host's estimate of the count (ilcc_api.cpp: full_pass_rule); a workgroup
// past the count returns, and items past G are left to k6_grid_cost_listed_rest.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k6_grid_cost_listed(Ctx c, GridPass pass) {
  K6_FULL_PASS_LDS(THREADS);
  if (blockIdx.x < min(*pass.work_count, c.n_frames * pass.blocks))   // (the list holds no more items than records)
    listed_item<THREADS>(c, pass, blockIdx.x, s_ij, s_hw, s_best, s_iters, s_cnt, s_ay, s_az, s_dead, s_live, &s_next);
}

// k6_grid_cost_listed_rest: the items from `first` (= the G of the launch in front of it) on, when the batch listed more than the host
// expected: workgroup b runs items first + b, first + b + (its grid), ... with a workgroup barrier in between, and retires behind
// them.  Every workgroup returns at once in the usual case.  (A kernel of its own because of its registers: around the item LOOP the
// compiler hoists everything that depends on the thread index alone and keeps it live through the body -- 93 VGPRs, five wavefronts
// per SIMD, or scratch when held to 72.  Which of the two kernels runs an item never shows in its record.)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k6_grid_cost_listed_rest(Ctx c, GridPass pass, uint32_t first) {
  K6_FULL_PASS_LDS(THREADS);
  const uint32_t n_items = min(*pass.work_count, c.n_frames * pass.blocks);
  for (uint32_t i = first + blockIdx.x; i < n_items; i += gridDim.x) {
    listed_item<THREADS>(c, pass, i, s_ij, s_hw, s_best, s_iters, s_cnt, s_ay, s_az, s_dead, s_live, &s_next);
    __syncthreads();   // the next item reuses the workgroup's LDS (thread 0 reads the wavefronts' bests last)
  }
}
#undef K6_FULL_PASS_LDS

// -DILCC_K6_ISA_PROBE (tools/k6_isa_count.sh): the two terms alone, N chained calls on N different points per kernel.  The
// VALU instructions of ONE evaluation = (instructions of the N = 3 kernel - instructions of the N = 1 kernel) / 2 -- counted
// by the script in the gfx950 assembly of THIS file with the library's own compiler flags, so bench.py's credit per executed
// evaluation is regenerated, not asserted.
#ifdef ILCC_K6_ISA_PROBE
template <int N, bool BORDER>
__global__ void k6_isa_probe(const float* __restrict__ pts, float ay, float az, float Wh, float Hh, float delta, float* out) {
  float A0 = 0.f, A1 = 0.f;
  const float lay = ay + (float)threadIdx.x, laz = az - (float)threadIdx.x;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const PointTerms p{pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]};
    if (BORDER)
      accumulate<true>(p, lay, laz, Wh, Hh, delta, A0, A1);
    else
      accumulate_interior(p, lay, laz, delta, A0, A1);
  }
  out[2 * threadIdx.x] = A0;
  out[2 * threadIdx.x + 1] = A1;
}
template <int N>
__global__ void k6_isa_probe_box(const float* __restrict__ pts, float alo, float ahi, float zlo, float zhi, float Wh, float Hh, float delta,
                                 float* out) {
  float lb = 0.f;
  const float t = (float)threadIdx.x;
#pragma unroll
  for (int k = 0; k < N; ++k) box_term(pts[2 * k], pts[2 * k], pts[2 * k + 1], pts[2 * k + 1], alo + t, ahi + t, zlo - t, zhi - t, Wh, Hh, delta, lb);
  out[threadIdx.x] = lb;
}
template __global__ void k6_isa_probe_box<1>(const float*, float, float, float, float, float, float, float, float*);
template __global__ void k6_isa_probe_box<3>(const float*, float, float, float, float, float, float, float, float*);
template __global__ void k6_isa_probe<1, true>(const float*, float, float, float, float, float, float*);
template __global__ void k6_isa_probe<3, true>(const float*, float, float, float, float, float, float*);
template __global__ void k6_isa_probe<1, false>(const float*, float, float, float, float, float, float*);
template __global__ void k6_isa_probe<3, false>(const float*, float, float, float, float, float, float*);
#endif

#ifdef ILCC_K6_TIMING
extern "C" int ilcc_debug_k6_profile(unsigned long long* out16, int clear) {
  static std::vector<unsigned long long> host((size_t)kProfWaves * kProfWords);
  if (hipMemcpyFromSymbol(host.data(), HIP_SYMBOL(k6_prof), host.size() * sizeof(unsigned long long)) != hipSuccess) return -1;
  for (int k = 0; k < 16; ++k) out16[k] = 0;
  for (size_t w = 0; w < (size_t)kProfWaves; ++w)
    for (int k = 0; k < kProfWords; ++k) out16[k] += host[w * kProfWords + k];
  if (clear) {
    std::fill(host.begin(), host.end(), 0ull);
    if (hipMemcpyToSymbol(HIP_SYMBOL(k6_prof), host.data(), host.size() * sizeof(unsigned long long)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

// executed-work unit of Ctx::grid_iters: one count = one point x one 16-candidate tile
uint32_t grid_cost_evals_per_count() { return kTile * kTile; }

// allow > 64 KiB of dynamic LDS (raise_grid_lds_limit, k6_common.h) in every K6 file.  Called by ilcc_create for the handle's device.
hipError_t set_kernel_attributes_k6() {
  hipError_t e = raise_grid_lds_limit({(const void*)k6_grid_cost<true, true, false, kGridThreads>, (const void*)k6_grid_cost<true, false, false, kGridThreads>,
                       (const void*)k6_grid_cost<false, true, false, kGridThreads>, (const void*)k6_grid_cost<false, false, false, kGridThreads>,
                       (const void*)k6_grid_cost<true, false, true, kGridThreads>,  (const void*)k6_grid_cost<false, false, true, kGridThreads>,
                       (const void*)k6_grid_cost<true, false, true, kGridThreadsLarge>, (const void*)k6_grid_cost_listed<kGridThreads>,
                       (const void*)k6_grid_cost_listed<kGridThreadsLarge>, (const void*)k6_grid_cost_listed_rest<kGridThreads>,
                       (const void*)k6_grid_cost_listed_rest<kGridThreadsLarge>});
  if (e == hipSuccess) e = set_kernel_attributes_k6_group_prepass();
  if (e == hipSuccess) e = set_kernel_attributes_k6_locate();
  return e;
}

void launch_grid_cost(const Ctx& c, const GridPass& pass, hipStream_t s, int32_t use_oob, float* cost_volume, bool prune) {
  const dim3 grid(pass.blocks, c.n_frames), block(kGridThreads);
  const size_t lds = grid_lds_bytes(c.grid_lds_points, pass.t.n_ty, pass.t.n_tz);
  // the diagnostic volume is always a complete evaluation (no pruning)
  if (cost_volume) {
    if (use_oob)
      hipLaunchKernelGGL((k6_grid_cost<true, true, false, kGridThreads>), grid, block, lds, s, c, pass, cost_volume);
    else
      hipLaunchKernelGGL((k6_grid_cost<false, true, false, kGridThreads>), grid, block, lds, s, c, pass, cost_volume);
  } else if (prune) {
    if (use_oob && c.grid_lds_points > (uint32_t)kGridLargeFrom)   // the pipeline's launches on large frames
      hipLaunchKernelGGL((k6_grid_cost<true, false, true, kGridThreadsLarge>), grid, dim3(kGridThreadsLarge), lds, s, c, pass, cost_volume);
    else if (use_oob)
      hipLaunchKernelGGL((k6_grid_cost<true, false, true, kGridThreads>), grid, block, lds, s, c, pass, cost_volume);
    else
      hipLaunchKernelGGL((k6_grid_cost<false, false, true, kGridThreads>), grid, block, lds, s, c, pass, cost_volume);
  } else {
    if (use_oob)
      hipLaunchKernelGGL((k6_grid_cost<true, false, false, kGridThreads>), grid, block, lds, s, c, pass, cost_volume);
    else
      hipLaunchKernelGGL((k6_grid_cost<false, false, false, kGridThreads>), grid, block, lds, s, c, pass, cost_volume);
  }
}

// the pipeline's full pass (pruning, out-of-board term) on the items k6_group_prepass listed: `workgroups` (>= 1) of
// k6_grid_cost_listed for the first as many items, and, unless that is one per record, kListedRest of k6_grid_cost_listed_rest for
// whatever the batch lists beyond them
constexpr uint32_t kListedRest = 1024;   // four per compute unit: enough to keep the chip busy on a batch the host's estimate missed
void launch_grid_cost_listed(const Ctx& c, const GridPass& pass, hipStream_t s, uint32_t workgroups) {
  const size_t lds = grid_lds_bytes(c.grid_lds_points, pass.t.n_ty, pass.t.n_tz);
  const bool large = c.grid_lds_points > (uint32_t)kGridLargeFrom;
  const dim3 block(large ? kGridThreadsLarge : kGridThreads);
  if (large)
    hipLaunchKernelGGL((k6_grid_cost_listed<kGridThreadsLarge>), dim3(workgroups), block, lds, s, c, pass);
  else
    hipLaunchKernelGGL((k6_grid_cost_listed<kGridThreads>), dim3(workgroups), block, lds, s, c, pass);
  const uint32_t records = c.n_frames * pass.blocks;
  if (workgroups >= records) return;
  const dim3 rest(records - workgroups < kListedRest ? records - workgroups : kListedRest);
  if (large)
    hipLaunchKernelGGL((k6_grid_cost_listed_rest<kGridThreadsLarge>), rest, block, lds, s, c, pass, workgroups);
  else
    hipLaunchKernelGGL((k6_grid_cost_listed_rest<kGridThreads>), rest, block, lds, s, c, pass, workgroups);
}

}  // namespace ilcc
