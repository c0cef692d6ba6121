// K7r pattern_refine (ILCC_SOLVER_GRID): one 192-thread workgroup (three wavefronts, one per theta of the stencil) per frame.  Starts at the K6 grid argmin
//      (near ties of the fp32 grid pass are first re-ordered on exact fixed-point costs), then a monotone
//      pattern search on the pass-A cost and a check of the eight neighbouring basins -- the same
//      specification as the oracle's orc_pattern_refine, bit for bit: every point's term is computed in
//      fp64 exactly like the oracle's, rounded to a multiple of 2^-40 and summed as an INTEGER, so the
//      parallel reduction cannot change a single decision.
// The REFERENCE_LOCAL mode's solver is K7a (k7a_local_solve.hip); K7b (k7b_corners.hip) turns either solver's records into corners.
#include <climits>
#include <type_traits>

#include "k7_common.h"

#ifdef ILCC_K7R_TIMING
#include <algorithm>
#include <vector>
#endif

namespace ilcc {

// -DILCC_K7R_TIMING: where a K7r wavefront's cycles go (cycle counter stamps around the phases of its life), one record per
// wavefront in k7r_prof[], read back through ilcc_debug_k7r_profile (tools/dev_k7r_phases.py).  Without the switch the stamps
// and the record compile away.
enum RefineProfSlot {
  kProfWritten = 0,   // 1: the record was written
  kProfSetup,         // staging + grid_argmin + recount_near_ties + first_round_is_settled
  kProfTrips,         // silence-test trips of the pattern rounds (the walk less its queued evaluations)
  kProfEvals,         // queued evaluations (and the walks of sweeps that skip nothing)
  kProfReduce,        // row reduction + LDS atomics
  kProfBarrier,       // waiting at the two barriers of a pattern round's sweep
  kProfDecide,        // decision step
  kProfBasin,         // basin checks: their sweeps, barriers and decisions
  kProfLife,          // entry to record
  kProfRounds,        // pattern rounds swept
  kProfTripCount,     // silence-test trips
  kProfQueued,        // points queued for evaluation
  kProfFrame,
  kProfWave,
  kProfWords = 16
};
#ifdef ILCC_K7R_TIMING
constexpr int kRefineProfWaves = 1 << 14;
__device__ unsigned long long k7r_prof[kRefineProfWaves * kProfWords];
#define K7R_STAMP(name) const unsigned long long name = __builtin_readcyclecounter()
#define K7R_SPENT(fr, slot, from, to) ((fr).prof[slot] += (to) - (from))
#define K7R_COUNT(fr, slot, k) ((fr).prof[slot] += (unsigned long long)(k))
#else
#define K7R_STAMP(name)
#define K7R_SPENT(fr, slot, from, to)
#define K7R_COUNT(fr, slot, k)
#endif

constexpr double kCostQOne = 1099511627776.0;   // 2^40: quantum of the fixed-point cost (oracle: ORC_COST_Q_ONE)
// wavefronts of the K7r workgroup: kRefineThreads / 64 in large batches, kRefineThreadsSmallBatch / 64 in small ones (the
// sums are integers: the split of the points over wavefronts cannot change a total)
#define kRefineWaves ((int)(blockDim.x >> 6))
// the 3-theta stencil gives every theta kRefineWaves / 3 wavefronts: fewer than 3 wavefronts would leave a theta without
// any (all 27 sums 0 -- a silently wrong refinement, not a build error), and the candidate lists are written by the first
// kRefineList threads
static_assert(kRefineThreads % ILCC_WAVE == 0 && kRefineThreads / ILCC_WAVE >= 3 && kRefineThreads >= kRefineList &&
              kRefineThreadsSmallBatch % (3 * ILCC_WAVE) == 0,
              "ILCC_K7R_THREADS must be a multiple of 64, at least 192");
constexpr float kBorderRisk = 4e-6f;             // squares: a board coordinate this close to an integer may be classified differently in fp32 (K6) and fp64
constexpr int32_t kNoTheta = INT32_MIN;         // candidate whose theta lies outside the lattice table: never evaluated

struct RCand {
  int32_t q0, q1, q2, phase;   // lattice coordinates (theta, ty, tz), topleftWhite
};
constexpr int kRefineWavesMax = kRefineThreadsSmallBatch / ILCC_WAVE;
constexpr double kExactDoubleSum = 9007199254740992.0;   // 2^53: a sum of non-negative integers below it was added exactly in double
constexpr int kActQueue = 128;                   // per-wavefront queue of active point indices: < 64 left over + <= 64 pushed
struct RefineShared {
  RCand cand[kRefineList];
  GridPartial meta[kRefineList];                 // near-tie recount: fp32 cost, d2, flat of the listed candidates
  unsigned long long acc[3][kRefineList];        // fixed-point sums, three rotating sets (sweep_begin / sweep_end)
  uint32_t queue[kRefineWavesMax][kActQueue];    // stencil_sweep: the points whose nine terms are not provably all zero
};

struct RefineState {
  int32_t lat[3];
  int32_t phase, rounds, hops, capped;
  int32_t skip_first;   // the start is the exhaustive grid's argmin with all 26 grid neighbours inside the grid (see pattern_refine)
  long long cost, alt;
};

__device__ __forceinline__ bool partial_less(const GridPartial& a, const GridPartial& b) {
  return a.cost < b.cost || (a.cost == b.cost && (a.d2 < b.d2 || (a.d2 == b.d2 && a.flat < b.flat)));
}

// ------------------------------------------------------------------ the lattice and the board
// The search lattice: every grid step of K6's tables divided into `div` lattice steps.  The one place that maps lattice
// coordinates to parameter values and a flat grid index to coordinates.
struct GridCell {
  int gk, ga, gb;   // indices into the grid tables (theta, ty, tz)
  RCand at;         // the same candidate in lattice coordinates, with its colour phase
};
struct Lattice {
  const Ctx& c;
  int div;                      // refine_div, or 1 without refinement
  double u_th, u_ty, u_tz;      // one lattice step: the grid's step / div
  __device__ __forceinline__ explicit Lattice(const Ctx& ctx) : c(ctx), div(ctx.p.refine_div > 0 ? ctx.p.refine_div : 1) {
    u_th = c.p.th_step / (double)div;
    u_ty = c.p.ty_step / (double)div;
    u_tz = c.p.tz_step / (double)div;
  }
  __device__ __forceinline__ double theta(int32_t q) const { return c.p.th_min + (double)q * u_th; }
  __device__ __forceinline__ double ty(int32_t q) const { return c.p.ty_min + (double)q * u_ty; }
  __device__ __forceinline__ double tz(int32_t q) const { return c.p.tz_min + (double)q * u_tz; }
  // q0 itself where the table of cos / sin has it, else kNoTheta
  __device__ __forceinline__ int32_t theta_or_none(int q0) const { return (q0 < c.th_lat_lo || q0 > c.th_lat_hi) ? kNoTheta : q0; }
  __device__ __forceinline__ double2 cs(int32_t q0) const { return c.th_lattice[q0 - c.th_lat_lo]; }
  // flat = ((k * n_ty + a) * n_tz + b) * 2 + phase (GridPartial::flat)
  __device__ __forceinline__ GridCell from_flat(uint32_t flat) const {
    const uint32_t cell = flat >> 1, n_ty = (uint32_t)c.p.n_ty, n_tz = (uint32_t)c.p.n_tz;
    GridCell g;
    g.gk = (int)(cell / (n_tz * n_ty));
    g.ga = (int)((cell / n_tz) % n_ty);
    g.gb = (int)(cell % n_tz);
    g.at = RCand{g.gk * div, g.ga * div, g.gb * div, (int32_t)(flat & 1u)};
    return g;
  }
};

struct Board {
  double W, H, g, delta;
  double inv_g;   // the coordinate is scaled by RN(1 / g), not divided by g (oracle: term_q)
};
__device__ __forceinline__ Board make_board(const ilcc_params& p) {
  return Board{(double)p.board_w, (double)p.board_h, p.grid_length, p.huber_delta, 1.0 / p.grid_length};
}
// board coordinates (in squares) of the labelled point v under the rotation cs = (cos, sin) and the translation (x1, x2):
// THE expression of the fixed-point cost -- the sweeps and the silence test all evaluate a point through it
struct BoardIJ {
  double i, j;
};
__device__ __forceinline__ BoardIJ board_ij(const Board& bd, double2 cs, double x1, double x2, float2 v) {
  const double y = (double)v.x, z = (double)v.y;
  const double ry = cs.x * y - cs.y * z;
  const double rz = cs.y * y + cs.x * z;
  return BoardIJ{((ry + x1) + bd.W * bd.g / 2.0) * bd.inv_g, ((rz + x2) + bd.H * bd.g / 2.0) * bd.inv_g};
}

// ------------------------------------------------------------------ the fixed-point cost
// The fixed-point cost's per-point term, operation for operation the oracle's term_q (oracle/ilcc_oracle.c): the
// functor's residual (Optimization.h:31-107) with the grid coordinate scaled by 1/g (computed once) instead of divided
// by g, and Huber's rho taken on r directly instead of through sqrt(r^2) -- no fp64 division or square root per
// point.  AxisTerms = everything the residual needs from one axis (v = i, n = W or v = j, n = H), so that the nine
// (ty, tz) combinations of a stencil share the three i's and three j's.
struct AxisTerms {
  double in_dist;    // min(frac, 1 - frac) as :70-78 compute it
  double out_dist;   // min(|v|, |v - n|) as :86-97 compute it
  bool inside;       // 0 < v < n (strict, :48-49)
  bool odd;          // floor(v) is odd
};
__device__ __forceinline__ AxisTerms axis_terms(double v, double n) {
  AxisTerms t;
  t.inside = v > 0 && v < n;
  const double fl = floor(v);
  // (floor(v) is odd) from the integer: the same truth value as `fl != floor(fl / 2) * 2` for every |v| < 2^31 -- board
  // coordinates are a few units -- at a quarter of the fp64 operations
  t.odd = (((int)fl) & 1) != 0;
  const double fr = v - fl;
  t.in_dist = (fr > 0.5) ? (fl + 1.0) - v : fr;
  t.out_dist = fmin(fabs(v), fabs(v - n));   // == (|v| < |v - n|) ? |v| : |v - n| for finite v
  return t;
}
// rint(1/2 rho * 2^40) as a double (an integer < 2^53: sums of a few of them are exact in double, too)
__device__ __forceinline__ double term_q(const AxisTerms& ai, const AxisTerms& aj, bool tlw, bool laser_white, double delta) {
  double res = 0.0;
  if (ai.inside && aj.inside) {
    const bool white = (ai.odd == aj.odd) ? tlw : !tlw;     // both even or both odd -> topleftWhite (:53-61)
    if (laser_white != white) res = ai.in_dist + aj.in_dist;
  } else {
    res = ai.out_dist + aj.out_dist;                        // useOutofBoard (pass-A cost)
  }
  const double r0 = (res > delta) ? 2.0 * delta * res - delta * delta : res * res;
  return rint(r0 * (0.5 * kCostQOne));
}

// ------------------------------------------------------------------ sweeps over a frame's points
// What the steps of one frame's refinement work on.  Every thread of the workgroup holds the same values.
struct Frame {
  const Ctx& c;
  Board bd;
  Lattice lat;
  const float2* yz;     // the frame's n labelled points: global memory, or LDS once staged
  const uint8_t* lab;
  uint32_t n;
  RefineShared& sh;
  int sweep;            // sweeps run so far
#ifdef ILCC_K7R_TIMING
  unsigned long long prof[kProfWords];   // this wavefront's record (begin_frame zeroes it)
#endif
};
// (zeroes the first sweep's acc set: the caller's barrier publishes it)
__device__ __forceinline__ Frame begin_frame(const Ctx& c, RefineShared& sh, const float2* yz, const uint8_t* lab, uint32_t n) {
  if (threadIdx.x < kRefineList) sh.acc[0][threadIdx.x] = 0ull;
  return Frame{c, make_board(c.p), Lattice(c), yz, lab, n, sh, 0};
}

// The rotating acc sets: sweep s adds into set s % 3, which sweep s - 1 zeroed (begin_frame the first), and zeroes set
// (s + 1) % 3, whose totals (sweep s - 2's) every thread read before it entered sweep s - 1 -- so one barrier in front of the
// adds and one behind them are all a sweep needs, and a caller may read a sweep's totals until the next sweep but one
// begins.  Returns the index of the set that will hold this sweep's totals.
__device__ __forceinline__ int sweep_begin(Frame& fr) {
  if (threadIdx.x < kRefineList) fr.sh.acc[(fr.sweep + 1) % 3][threadIdx.x] = 0ull;
  __syncthreads();   // candidates (written by the caller) and this sweep's zeroed set are visible
  return fr.sweep % 3;
}
__device__ __forceinline__ void sweep_end(Frame& fr) {
  __syncthreads();
  ++fr.sweep;
}

// One sweep over the frame's labelled points for the n_cand (<= 32) candidates in sh.cand.  lane -> (candidate,
// slice): every lane walks its slice of the points for ONE candidate and adds its integer partial sum to the
// candidate's LDS word -- no cross-lane reduction, and the result cannot depend on who adds first.
// Returns the index of the acc set that holds the totals.
__device__ __forceinline__ int refine_sweep(Frame& fr, int n_cand) {
  const int buf = sweep_begin(fr);
  const int lane = lane_id();
  const int slices = ILCC_WAVE / n_cand;
  const int cand = lane % n_cand, slice = lane / n_cand;
  if (slice < slices) {
    const RCand cd = fr.sh.cand[cand];
    if (cd.q0 != kNoTheta) {
      const double2 cs = fr.lat.cs(cd.q0);
      const double x1 = fr.lat.ty(cd.q1), x2 = fr.lat.tz(cd.q2);
      const bool tlw = cd.phase != 0;
      long long sum = 0;
      for (uint32_t p = (uint32_t)(wave_id() * slices + slice); p < fr.n; p += (uint32_t)(kRefineWaves * slices)) {
        const BoardIJ at = board_ij(fr.bd, cs, x1, x2, fr.yz[p]);
        const AxisTerms ai = axis_terms(at.i, fr.bd.W);
        const AxisTerms aj = axis_terms(at.j, fr.bd.H);
        sum += (long long)term_q(ai, aj, tlw, fr.lab[p] != 0, fr.bd.delta);
      }
      atomicAdd(&fr.sh.acc[buf][cand], (unsigned long long)sum);
    }
  }
  sweep_end(fr);
  return buf;
}

// One sweep for a 3 x 3 x 3 (or 1 x 3 x 3) STENCIL of candidates: theta in th[0..n_th), ty in ty[0..3), tz in tz[0..3),
// colour phase = phase ^ (parity ? (a + b) & 1 : 0).  Wavefront w serves theta w % n_th; its lanes take points
// (slice, slice + n_slices, ...) and evaluate the 9 translations of each: rotation once, the per-axis terms of the
// three i's and three j's once, then 9 cheap combinations -- the same doubles as 27 independent term evaluations.
// Totals land in sh.acc[buf][theta * 9 + a * 3 + b].
//
// SILENT POINTS ARE SKIPPED (pattern-search rounds, parity == false).  Most labelled points sit in a square of their own
// colour, well away from its borders: their term is exactly 0 for the centre and for every neighbour of a fine-stride
// stencil.  A point is silent for this wavefront's theta when, by board_ij itself,
//   0 < i(ty[0]) and i(ty[2]) < W and floor(i(ty[0])) == floor(i(ty[2])),   the same for j, and its label is the cell's colour:
// ty[0] <= ty[1] <= ty[2] and every operation of board_ij is monotone in x, so i(ty[1]) lies between the two -- all three
// i's (and j's) are strictly inside the board and in ONE cell, all nine residuals are 0 and term_q(...) = rint(0) = 0.
// Points that fail the test (a fifth of the nine evaluations' cost) are queued per wavefront in LDS (a ballot compaction)
// and evaluated 64 at a time.  Sums are integers, so the totals are bit-identical to evaluating every point, as the oracle
// does.  On the bench's frames 75-95 % of the points are silent, depending on the stride.
__device__ __forceinline__ int stencil_sweep(Frame& fr, int n_th, const int32_t th[3], const int32_t ty[3], const int32_t tz[3],
                                             int phase, bool parity) {
  const Ctx& c = fr.c;
  const Board& bd = fr.bd;
  const float2* yz = fr.yz;
  const uint8_t* lab = fr.lab;
  const uint32_t n = fr.n;
  K7R_STAMP(t_begin);
  const int buf = sweep_begin(fr);
  K7R_STAMP(t_open);
  K7R_SPENT(fr, parity ? kProfBasin : kProfBarrier, t_begin, t_open);
  const int wid = __builtin_amdgcn_readfirstlane(wave_id());
  const int waves_per_theta = kRefineWaves / n_th;          // 3 wavefronts: one per theta of the stencil, or all three on the basin check's single theta
  const int it = wid % n_th, grp = wid / n_th;
  const int32_t q0 = th[it];
  if (grp < waves_per_theta && q0 != kNoTheta) {
    const int lane = lane_id();
    const double2 cs = fr.lat.cs(q0);
    double x1[3], x2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x1[k] = fr.lat.ty(ty[k]);
      x2[k] = fr.lat.tz(tz[k]);
    }
    // The lane's nine partial sums.  The terms are integers below 2^53, and a double adds integers exactly as long as the SUM
    // stays below 2^53 -- one fp64 add per term where an int64 sum costs a conversion (no 64-bit one in the ISA) and a carry.
    // Domain: a lane adds P = ceil(n / n_slices) terms (n_slices = 64 x the theta's wavefronts: 64 in the pattern rounds
    // of the 192-thread kernel, 192 in its basin check, 256 / 768 in small batches) of at most 2^39 rho(r), where
    // rho(r) = r^2 for r <= huber_delta, else 2 huber_delta r - huber_delta^2, and r is a point's distance from the board in
    // squares (the sum over y and z of its distance to the nearer outline, or at most 1 inside).  The doubles are exact when
    //   P x rho(r_max) < 2^14 = 16384:
    // the default delta = 0.1 with 28 800 points 2 m off a 0.15 m board gives 450 x 5.3; delta = 5 with 8 000 points
    // up to 0.9 m off gives 125 x 44.  Outside it (delta = 5, 28 800 points 1-2 m off: 450 x 191) a lane's sum passes 2^53
    // and an add may round.  That is DETECTED, not assumed away: the terms are >= 0, so the sums only grow and rounding is
    // monotone -- a lane whose final sum is below 2^53 never rounded.  A wavefront with a lane at or above 2^53 walks
    // its points again with int64 sums (the oracle's own arithmetic): the totals are the exact ones for every input.
    const uint32_t n_slices = (uint32_t)(waves_per_theta * ILCC_WAVE);
    // the silence test needs ty[0] <= ty[2] and tz[0] <= tz[2] (pattern-search rounds: centre -/+ stride, steps > 0)
    const bool skip_silent = !parity && ty[0] <= ty[1] && ty[1] <= ty[2] && tz[0] <= tz[1] && tz[1] <= tz[2] && c.p.ty_step > 0.0 && c.p.tz_step > 0.0;   // (monotone in BOTH steps: the middle value's cell lies between the outer two's)
    // one walk over this wavefront's points, the nine sums in acc[] (double: the fast form; long long: the exact one)
    auto walk = [&](auto* acc) {
      using Acc = std::remove_reference_t<decltype(acc[0])>;
#pragma unroll
      for (int e = 0; e < 9; ++e) acc[e] = (Acc)0;
      auto eval_point = [&](uint32_t p) {
        const float2 v = yz[p];
        const bool laser_white = lab[p] != 0;
        AxisTerms ai[3], aj[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const BoardIJ at = board_ij(bd, cs, x1[k], x2[k], v);
          ai[k] = axis_terms(at.i, bd.W);
          aj[k] = axis_terms(at.j, bd.H);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) {
            const bool tlw = ((phase ^ (parity ? ((a + b) & 1) : 0)) != 0);
            acc[a * 3 + b] += (Acc)term_q(ai[a], aj[b], tlw, laser_white, bd.delta);
          }
      };
      if (skip_silent) {
        uint32_t* queue = fr.sh.queue[wid];
        uint32_t head = 0, tail = 0;   // wave-uniform
        const bool tlw0 = phase != 0;
        for (uint32_t base = (uint32_t)(grp * ILCC_WAVE); base < n; base += n_slices) {
          const uint32_t p = base + (uint32_t)lane;
          bool active = false;
          if (p < n) {
            const float2 v = yz[p];
            const BoardIJ lo = board_ij(bd, cs, x1[0], x2[0], v), hi = board_ij(bd, cs, x1[2], x2[2], v);
            const double fi = floor(lo.i), fj = floor(lo.j);
            const bool one_cell = lo.i > 0 && hi.i < bd.W && lo.j > 0 && hi.j < bd.H && fi == floor(hi.i) && fj == floor(hi.j);
            const bool odd_i = (((int)fi) & 1) != 0, odd_j = (((int)fj) & 1) != 0;
            const bool white = (odd_i == odd_j) ? tlw0 : !tlw0;   // term_q's colour rule (:53-61)
            active = !(one_cell && (lab[p] != 0) == white);
          }
          const unsigned long long m = __ballot(active);
          K7R_COUNT(fr, kProfTripCount, 1);
          if (m != 0ull) {
            if (active) queue[(tail + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))) & (kActQueue - 1)] = p;
            tail += (uint32_t)__popcll(m);
            K7R_COUNT(fr, kProfQueued, __popcll(m));
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // one wavefront: LDS executes its instructions in order; keep the compiler from reordering
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            K7R_STAMP(t_drain);
            while (tail - head >= (uint32_t)ILCC_WAVE) {
              eval_point(queue[(head + (uint32_t)lane) & (kActQueue - 1)]);
              head += ILCC_WAVE;
            }
            K7R_STAMP(t_drained);
            K7R_SPENT(fr, kProfEvals, t_drain, t_drained);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the reads above before the next round's writes
            __builtin_amdgcn_wave_barrier();
          }
        }
        K7R_STAMP(t_rest);
        if ((uint32_t)lane < tail - head) eval_point(queue[(head + (uint32_t)lane) & (kActQueue - 1)]);
        K7R_STAMP(t_rested);
        K7R_SPENT(fr, kProfEvals, t_rest, t_rested);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // ... and before a second walk's
        __builtin_amdgcn_wave_barrier();
      } else {
        for (uint32_t p = (uint32_t)(grp * ILCC_WAVE + lane); p < n; p += n_slices) eval_point(p);
      }
    };
    unsigned long long tot[9];
    K7R_STAMP(t_walk);
    {
      double acc[9];
      walk(acc);
      bool rounded = false;
#pragma unroll
      for (int e = 0; e < 9; ++e) {
        rounded |= !(acc[e] < kExactDoubleSum);
        tot[e] = (unsigned long long)(long long)acc[e];
      }
      if (__ballot(rounded) != 0ull) {
        long long iacc[9];
        walk(iacc);
#pragma unroll
        for (int e = 0; e < 9; ++e) tot[e] = (unsigned long long)iacc[e];
      }
    }
    K7R_STAMP(t_walked);
    K7R_SPENT(fr, parity ? kProfBasin : kProfTrips, t_walk, t_walked);   // (the record takes the queued evaluations off the trips)
    // integer sums: any reduction order gives the same totals
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      // within the 16-lane rows only (plain DPP); the four rows then add their totals to the LDS word themselves -- the two
      // cross-row steps (permlane swaps and selects on both halves of a 64-bit value) cost more than three more atomics
      unsigned long long t = tot[e];
      t += xor_lane_u64<8>(t);
      t += xor_lane_u64<4>(t);
      t += xor_lane_u64<2>(t);
      t += xor_lane_u64<1>(t);
      if ((lane & 15) == 0) atomicAdd(&fr.sh.acc[buf][it * 9 + e], t);
    }
    K7R_STAMP(t_added);
    K7R_SPENT(fr, parity ? kProfBasin : kProfReduce, t_walked, t_added);
  }
  K7R_STAMP(t_close);
  sweep_end(fr);
  K7R_STAMP(t_end);
  K7R_SPENT(fr, parity ? kProfBasin : kProfBarrier, t_close, t_end);
  return buf;
}

// ------------------------------------------------------------------ the steps of a frame's refinement
// argmin over frame f's K6 partials: cost, then index distance to zero, then flat index (every wavefront repeats the same
// reduction: no broadcast needed).  flat == 0xFFFFFFFF: the grid search left no candidate
__device__ __forceinline__ GridPartial grid_argmin(const Ctx& c, uint32_t f) {
  const GridPartial* gp = c.partial + (uint64_t)f * c.grid_blocks;
  GridPartial b{__builtin_inff(), 0xFFFFFFFFu, 0xFFFFFFFFu, 0u};
  for (uint32_t k = lane_id(); k < c.grid_blocks; k += ILCC_WAVE) {
    const GridPartial t = gp[k];
    if (partial_less(t, b)) b = t;
  }
#pragma unroll
  for (int o = ILCC_WAVE / 2; o > 0; o >>= 1) {
    GridPartial t;
    t.cost = __shfl_xor(b.cost, o, ILCC_WAVE);
    t.d2 = __shfl_xor(b.d2, o, ILCC_WAVE);
    t.flat = __shfl_xor(b.flat, o, ILCC_WAVE);
    if (partial_less(t, b)) b = t;
  }
  return b;
}

// Near ties: fp32 sums of ~1e3 terms cannot order candidates whose costs agree to ~1e-6; the oracle orders them
// on exact fixed-point sums.  K6's full pass listed every candidate within kTieEps of the bound; recount the
// ones within kTieEps of the fp32 minimum b with the oracle's arithmetic and apply its tie-break to those values.
// Returns the number of listed ties; b becomes the oracle's pick.
__device__ __forceinline__ uint32_t recount_near_ties(Frame& fr, uint32_t f, GridPartial& b, int& flags) {
  const Ctx& c = fr.c;
  RefineShared& sh = fr.sh;
  if (c.tie_count == nullptr) return 0;
  const uint32_t n_ties = c.tie_count[f];
  if (n_ties > (uint32_t)kTieCap) {
    flags |= ILCC_FLAG_TIE_OVERFLOW;   // the list is incomplete: keep the (deterministic) fp32 argmin
    return n_ties;
  }
  const GridPartial* tl = c.tie_list + (uint64_t)f * kTieCap;
  const float window = b.cost * (1.f + kTieEps);
  uint32_t close = 0;
  for (uint32_t e = 0; e < n_ties; ++e) close += (tl[e].cost <= window && tl[e].flat != b.flat) ? 1u : 0u;
  if (close > 0) {   // uniform across the workgroup
    long long best_q = LLONG_MAX;
    GridPartial pick = b;
    int k = 0;
    for (uint32_t e = 0; e <= n_ties; ++e) {   // e == n_ties: the fp32 argmin itself
      const GridPartial t = (e < n_ties) ? tl[e] : b;
      const bool take = (t.cost <= window) && !(e < n_ties && t.flat == b.flat);
      if (take) {
        if (threadIdx.x == 0) {
          sh.cand[k] = fr.lat.from_flat(t.flat).at;
          sh.meta[k] = t;
        }
        ++k;
      }
      if (k == kRefineList || (e == n_ties && k > 0)) {
        const int bf = refine_sweep(fr, k);
        for (int j = 0; j < k; ++j) {
          const long long cq = (long long)sh.acc[bf][j];
          const GridPartial m = sh.meta[j];
          if (cq < best_q || (cq == best_q && (m.d2 < pick.d2 || (m.d2 == pick.d2 && m.flat < pick.flat)))) {
            best_q = cq;
            pick = m;
          }
        }
        k = 0;
        __syncthreads();   // every thread has read meta / cand before thread 0 refills them
      }
    }
    b = pick;
  }
  return n_ties;
}

// The first round of the first search looks at the 26 neighbours one GRID step away.  When they are all grid candidates,
// K6 has already ranked them: pruned ones cost more than (1 + 2e-5) x the minimum, completed ones within that window were
// re-ordered on exact costs by recount_near_ties -- none can be STRICTLY cheaper than the argmin, the round cannot move and
// is not evaluated (it still counts as a round: `rounds` stays the oracle's number).  Not when the near-tie list overflowed
// (the argmin is then the fp32 one).
// ... and not when K6's ranking of these 27 candidates cannot be trusted: K6 sums fp32 terms, and a point within fp32 rounding
// of a cell border under one of them may sit in the OTHER cell there -- its term then differs from the exact one by a whole
// residual, not by rounding, and "pruned => costs more" no longer follows.  The test below recomputes, with K6's own fp32
// expressions (its staging's rotation, its table values), the board coordinates of every labelled point under the 3 thetas
// x (3 + 3) axis translations of the neighbourhood and looks for one within 4e-6 square of an integer (fp32 and fp64 agree
// to ~1e-6 there).  None: every point is classified alike in fp32 and fp64 for all 27, their fp32 costs are the exact ones
// up to summation rounding (1e-6 relative, far inside the 2e-5 window) and the shortcut is sound.  Any: ILCC_FLAG_BORDER_RISK,
// and the round is evaluated like every other.
__device__ __forceinline__ bool first_round_is_settled(const Frame& fr, const GridCell& at, int& flags) {
  const Ctx& c = fr.c;
  const int gk = at.gk, ga = at.ga, gb = at.gb, n_ty = c.p.n_ty, n_tz = c.p.n_tz;
  bool risk = false;
  for (uint32_t i = threadIdx.x; i < fr.n; i += blockDim.x) {
    const float2 v = fr.yz[i];
#pragma unroll
    for (int dk = -1; dk <= 1; ++dk) {
      const int k = gk + dk;
      if (k < 0 || k >= c.p.n_th) continue;
      const float cth = c.grid.cth[k], sth = c.grid.sth[k];
      const float pi = fmaf(-sth, v.y, cth * v.x), pj = fmaf(cth, v.y, sth * v.x);   // = k6_grid_cost's staging
#pragma unroll
      for (int d = -1; d <= 1; ++d) {
        const int a = ga + d, b = gb + d;
        if (a >= 0 && a < n_ty) {
          const float x = pi + c.grid.ay[a];
          risk |= fabsf(x - rintf(x)) < kBorderRisk;
        }
        if (b >= 0 && b < n_tz) {
          const float x = pj + c.grid.az[b];
          risk |= fabsf(x - rintf(x)) < kBorderRisk;
        }
      }
    }
  }
  risk = __syncthreads_or(risk ? 1 : 0) != 0;
  if (risk) flags |= ILCC_FLAG_BORDER_RISK;
  return !risk && !(flags & ILCC_FLAG_TIE_OVERFLOW) && gk > 0 && gk < c.p.n_th - 1 && ga > 0 && ga < n_ty - 1 && gb > 0 && gb < n_tz - 1;
}

// The least (cost, key) pair of lanes 0..31, cost first and then key, returned wave-uniform: five register-only exchanges
// (comparisons of integers: the order of the reduction cannot change the pick).  Every wavefront runs it on its own copy, all
// 64 lanes active; lanes that hold no entry pass (LLONG_MAX, 0xFFFFFFFF).
template <int MASK>
__device__ __forceinline__ void argmin_step(long long& cost, uint32_t& key) {
  const long long oc = (long long)xor_lane_u64<MASK>((unsigned long long)cost);
  const uint32_t ok = xor_lane_u32<MASK>(key);
  const bool take = oc < cost || (oc == cost && ok < key);
  cost = take ? oc : cost;
  key = take ? ok : key;
}
__device__ __forceinline__ void argmin_lanes32(long long& cost, uint32_t& key) {
  argmin_step<16>(cost, key);
  argmin_step<8>(cost, key);
  argmin_step<4>(cost, key);
  argmin_step<2>(cost, key);
  argmin_step<1>(cost, key);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(unsigned long long)cost);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((unsigned long long)cost >> 32));
  cost = (long long)(((unsigned long long)hi << 32) | lo);
  key = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
}

// orc_pattern_refine from st.lat / st.phase (st.skip_first: see first_round_is_settled), executed redundantly (and
// identically) by every thread of the workgroup
__device__ __forceinline__ void pattern_refine(Frame& fr, RefineState& st) {
  const Ctx& c = fr.c;
  const RefineShared& sh = fr.sh;
  const bool refine = c.p.refine_div > 0;
  const int div = fr.lat.div;
  st.rounds = 0;
  st.hops = 0;
  st.capped = 0;
  st.cost = 0;
  st.alt = 0;
  for (;;) {
    int stride = div, r = 0;
    if (st.skip_first && refine && div >= 2 && c.p.refine_max_rounds >= 1) {   // (first search only: a hop restarts in full)
      stride = div >> 1;
      r = 1;
    }
    st.skip_first = 0;
    while (refine && stride >= 1 && r < c.p.refine_max_rounds) {
      int32_t th[3], ty[3], tz[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        th[k] = fr.lat.theta_or_none(st.lat[0] + (k - 1) * stride);
        ty[k] = st.lat[1] + (k - 1) * stride;
        tz[k] = st.lat[2] + (k - 1) * stride;
      }
      const int b = stencil_sweep(fr, 3, th, ty, tz, st.phase, false);
      K7R_STAMP(t_swept);
      // lane e < 27 holds neighbour e in (dk, da, db) order; the pick is the oracle's: lower cost, then nearer (smaller d2), then
      // first (lower e) -- the least (cost, d2 * 32 + e).  The centre and the thetas outside the table take no part; an entry
      // of LLONG_MAX is never taken, as in a loop that starts from it.
      const int le = min(lane_id(), 26);
      const int ldk = le / 9 - 1, lda = (le / 3) % 3 - 1, ldb = le % 3 - 1;
      const bool listed = lane_id() < 27 && le != 13 && fr.lat.theta_or_none(st.lat[0] + ldk * stride) != kNoTheta;
      long long bc = listed ? (long long)sh.acc[b][le] : LLONG_MAX;
      uint32_t bkey = listed ? (uint32_t)((ldk * ldk + lda * lda + ldb * ldb) * 32 + le) : 0xFFFFFFFFu;
      argmin_lanes32(bc, bkey);
      const int be = (bc == LLONG_MAX) ? -1 : (int)(bkey & 31u);
      const long long centre = (long long)sh.acc[b][13];
      ++r;
      if (be >= 0 && bc < centre) {
        st.lat[0] += (be / 9 - 1) * stride;
        st.lat[1] += ((be / 3) % 3 - 1) * stride;
        st.lat[2] += (be % 3 - 1) * stride;
      } else {
        stride >>= 1;
      }
      K7R_STAMP(t_decided);
      K7R_SPENT(fr, kProfDecide, t_swept, t_decided);
      K7R_COUNT(fr, kProfRounds, 1);
    }
    st.rounds += r;
    if (refine && stride >= 1) st.capped = 1;   // left the loop on the round cap, not on the stride
    // the eight neighbouring basins (one square along y and/or z; an odd shift swaps the colours) + the centre
    const int32_t th1[3] = {st.lat[0], kNoTheta, kNoTheta};
    const int32_t hy[3] = {st.lat[1] - c.refine_hop_y, st.lat[1], st.lat[1] + c.refine_hop_y};
    const int32_t hz[3] = {st.lat[2] - c.refine_hop_z, st.lat[2], st.lat[2] + c.refine_hop_z};
    // ((da + db) & 1 with da, db in {-1, 0, 1} == (a + b) & 1 with a = da + 1, b = db + 1)
    const int b = stencil_sweep(fr, 1, th1, hy, hz, st.phase, true);
    K7R_STAMP(t_basin);
    st.cost = (long long)sh.acc[b][4];
    // lane e < 9 holds basin e; the cheapest of the eight neighbours, the first of equals: the least (cost, e)
    const int he = min(lane_id(), 8);
    const bool neighbour = lane_id() < 9 && he != 4;
    long long alt = neighbour ? (long long)sh.acc[b][he] : LLONG_MAX;
    uint32_t akey = neighbour ? (uint32_t)he : 0xFFFFFFFFu;
    argmin_lanes32(alt, akey);
    const int ae = (int)(akey & 15u);   // (read only where alt < st.cost: a neighbour's)
    st.alt = alt;
    K7R_STAMP(t_basin_read);
    K7R_SPENT(fr, kProfBasin, t_basin, t_basin_read);
    if (alt < st.cost && st.hops < 2 && refine) {
      const int da = ae / 3 - 1, db = ae % 3 - 1;
      ++st.hops;
      st.lat[1] += da * c.refine_hop_y;
      st.lat[2] += db * c.refine_hop_z;
      st.phase ^= (da + db) & 1;
      continue;
    }
    break;
  }
}

__device__ __forceinline__ RefineState start_at(const RCand& at, bool skip_first) {
  RefineState st;
  st.lat[0] = at.q0;
  st.lat[1] = at.q1;
  st.lat[2] = at.q2;
  st.phase = at.phase;
  st.skip_first = skip_first ? 1 : 0;
  return st;
}

__device__ __forceinline__ void store_record(const Lattice& lat, const RefineState& st, int flags, uint32_t n_ties, SolveRec* out) {
  out->x[0] = lat.theta(st.lat[0]);
  out->x[1] = lat.ty(st.lat[1]);
  out->x[2] = lat.tz(st.lat[2]);
  out->cost_a = out->sel = (double)st.cost / kCostQOne;
  out->cost_b = (double)st.alt / kCostQOne;
  out->margin = ((double)st.alt - (double)st.cost) / (double)(st.cost > 0 ? st.cost : 1);
  out->iters_a = st.rounds;
  out->iters_b = st.hops;
  out->phase = st.phase;
  out->valid = 1;
  out->flags = flags | (st.capped ? ILCC_FLAG_REFINE_CAPPED : 0);
  out->ties = (int32_t)n_ties;
  out->cost_q = st.cost;
  out->alt_q = st.alt;
}

// (LDS_POINTS is a template argument, not a pointer select: each instantiation shows the compiler the address space of the
// points every sweep reads)
template <bool LDS_POINTS>
__device__ __forceinline__ void refine_frame(const Ctx& c, SolveRec* rec, const StagedPoints& lds, RefineShared& sh) {
  K7R_STAMP(t_entry);
  const uint32_t f = blockIdx.x;
  const uint64_t beg = c.off[f];
  SolveRec* out = &rec[2 * f];
  Frame fr = begin_frame(c, sh, c.yz + beg, c.lab + beg, c.n_lab[f]);
  if (LDS_POINTS) {
    for (uint32_t i = threadIdx.x; i < fr.n; i += blockDim.x) {
      lds.yz[i] = fr.yz[i];
      lds.lab[i] = fr.lab[i];
    }
    fr.yz = lds.yz;
    fr.lab = lds.lab;
  }
  __syncthreads();

  GridPartial b = grid_argmin(c, f);
  if (b.flat == 0xFFFFFFFFu) {
    if (threadIdx.x == 0) out->valid = 0;
    return;
  }
  int flags = 0;
  const uint32_t n_ties = recount_near_ties(fr, f, b, flags);
  if (threadIdx.x == 0) {
    c.res[f].grid_index = (int32_t)b.flat;
    c.res[f].grid_cost = b.cost;
  }
  const GridCell start = fr.lat.from_flat(b.flat);
  RefineState st = start_at(start.at, first_round_is_settled(fr, start, flags));
  K7R_STAMP(t_start);
  pattern_refine(fr, st);
  if (threadIdx.x == 0) store_record(fr.lat, st, flags, n_ties, out);
#ifdef ILCC_K7R_TIMING
  if (lane_id() == 0) {   // one record per wavefront: the last batch that ran frame f keeps it
    const unsigned long long t_done = __builtin_readcyclecounter();
    const uint32_t wid = (uint32_t)wave_id();
    unsigned long long* o = k7r_prof + (size_t)((f * (uint32_t)kRefineWaves + wid) & (uint32_t)(kRefineProfWaves - 1)) * kProfWords;
    fr.prof[kProfWritten] = 1ull;
    fr.prof[kProfSetup] = t_start - t_entry;
    fr.prof[kProfTrips] -= fr.prof[kProfEvals];   // (the walk of a pattern round = its trips + its queued evaluations)
    fr.prof[kProfLife] = t_done - t_entry;
    fr.prof[kProfFrame] = f;
    fr.prof[kProfWave] = wid;
    for (int k = 0; k < kProfWords; ++k) o[k] = fr.prof[k];
  }
#endif
}

__global__ __launch_bounds__(kRefineThreadsSmallBatch) void k7r_pattern_refine(Ctx c, SolveRec* rec) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ RefineShared sh;
  const uint32_t f = blockIdx.x;
  if (c.res[f].status != ILCC_OK) {
    if (threadIdx.x == 0) rec[2 * f].valid = 0;
    return;
  }
  const StagedPoints lds = staged_points(smem, c.grid_lds_points, 1, 0);
  if (c.n_lab[f] <= c.grid_lds_points)
    refine_frame<true>(c, rec, lds, sh);
  else
    refine_frame<false>(c, rec, lds, sh);
}

// test entry: the refinement alone on frame 0's labelled points (global memory), start given by the caller
__global__ __launch_bounds__(kRefineThreads) void k7r_pattern_refine_test(Ctx c, RefineOut* io) {
  __shared__ RefineShared sh;
  Frame fr = begin_frame(c, sh, c.yz, c.lab, c.n_lab[0]);
  // (skip_first = false: an arbitrary start, nothing is known about its grid neighbours)
  RefineState st = start_at(RCand{io->lat[0], io->lat[1], io->lat[2], io->phase}, false);
  __syncthreads();
  pattern_refine(fr, st);
  if (threadIdx.x == 0) {
    io->lat[0] = st.lat[0];
    io->lat[1] = st.lat[1];
    io->lat[2] = st.lat[2];
    io->phase = st.phase;
    io->rounds = st.rounds;
    io->hops = st.hops;
    io->cost_q = st.cost;
    io->alt_q = st.alt;
  }
}

hipError_t set_kernel_attributes_k7r() {
  return hipFuncSetAttribute((const void*)k7r_pattern_refine, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)staged_points_bytes(kGridLdsPointsMax, 1));
}

void launch_pattern_refine(const Ctx& c, hipStream_t s) {
  const int threads = c.n_frames <= (uint32_t)kSmallBatchFrames ? kRefineThreadsSmallBatch : kRefineThreads;
  hipLaunchKernelGGL(k7r_pattern_refine, dim3(c.n_frames), dim3(threads), staged_points_bytes(c.grid_lds_points, 1), s, c, c.solve_rec);
}

void launch_pattern_refine_test(const Ctx& c, hipStream_t s, RefineOut* d_io) {
  hipLaunchKernelGGL(k7r_pattern_refine_test, dim3(1), dim3(kRefineThreads), 0, s, c, d_io);
}

#ifdef ILCC_K7R_TIMING
// out: the written records (kProfWords words each, RefineProfSlot order), at most cap_records of them; returns their number
extern "C" int ilcc_debug_k7r_profile(unsigned long long* out, int cap_records, int clear) {
  static std::vector<unsigned long long> host((size_t)kRefineProfWaves * kProfWords);
  if (hipMemcpyFromSymbol(host.data(), HIP_SYMBOL(k7r_prof), host.size() * sizeof(unsigned long long)) != hipSuccess) return -1;
  int n = 0;
  for (size_t w = 0; w < (size_t)kRefineProfWaves && n < cap_records; ++w)
    if (host[w * kProfWords + kProfWritten] != 0ull) {
      std::copy(host.begin() + w * kProfWords, host.begin() + (w + 1) * kProfWords, out + (size_t)n * kProfWords);
      ++n;
    }
  if (clear) {
    std::fill(host.begin(), host.end(), 0ull);
    if (hipMemcpyToSymbol(HIP_SYMBOL(k7r_prof), host.data(), host.size() * sizeof(unsigned long long)) != hipSuccess) return -1;
  }
  return n;
}
#endif

}  // namespace ilcc
