// k6_common.h -- what more than one of the K6 files needs (k6_grid_cost.hip, k6_group_prepass.hip, k6_locate.hip, and ilcc_api.cpp
// for the layouts' sizes): the tuned constants, the lane reductions and argmin records, the walk layout's accessors, the term
// functions, the box pre-pass's rounds, and the LDS layouts and samples the host and the kernels must agree on -- each written
// once, after the model of staged_points / staged_points_bytes in k7_common.h.  No kernel bodies live here.
#pragma once

#include "ilcc_internal.h"
#include "k5w_walk_order.h"
#include <initializer_list>
#include <type_traits>

namespace ilcc {

// Tuned constants (the measurements behind each value are in DESIGN.md section 4, "K6 tuning record")
#ifndef ILCC_SEED_SHIFT
#define ILCC_SEED_SHIFT 4   // round 3: an eighth (1/2: 323 k, 1/4: 331 k, 1/8: 335 k, 1/16: 329 k frames/s); round 6, with the bound anchored on all points anyway: 1/4: 1 247 k, 1/8: 1 282 k (locate 0.187 ms alone), 1/16 = the 128-point floor on VLP-16 frames: 1 288 k (0.166 ms), 1/32: the same; config 5 unchanged (90-91 k)
#endif
constexpr int kSeedShift = ILCC_SEED_SHIFT;     // subsampled (locate) launches walk M >> kSeedShift positions, at least GridPass::walk_limit
constexpr int kTile = 4;          // 4 x 4 candidates per wavefront; lane = ((a << 2) | b) << 2 | slice
constexpr int kSlices = 4;        // lanes (one quad) sharing a candidate, each on every 4th point of the walk
constexpr int kUnroll = 2;        // points per lane and block of the generic walk
constexpr int kStep = kSlices * kUnroll;
// the 512-thread instance of the full pass and of the common pre-pass (handles staging above kGridLargeFrom points), where the build has one
template <int THREADS>
constexpr bool kIsLargeInstance = THREADS == kGridThreadsLarge && kGridThreadsLarge != kGridThreads;
constexpr int kBoxShiftSmall = 3;   // box pre-pass: at least 1/8 of the frame's labelled points per tile (and at least GridPass::box_points) ...
constexpr int kBoxShiftLarge = 2;   // ... 1/4 in the 512-thread instance (frames of several thousand labelled points)
template <int THREADS>
constexpr int kBoxShiftOf = kIsLargeInstance<THREADS> ? kBoxShiftLarge : kBoxShiftSmall;
// the common pre-pass (k6_group_prepass) looks at M >> kGroupShift points of the rim-first walk: a quarter in the 256-thread instance, half in
// the 512-thread one (twice what each theta's own pre-pass looks at)
#ifndef ILCC_GROUP_SHIFT_SMALL
#define ILCC_GROUP_SHIFT_SMALL 2   // round 6 (the only filter in front of the walk now), k frames/s: 1 (half): 1 284-1 295, 2: 1 285-1 288, 3: 1 199-1 222
#endif
#ifndef ILCC_GROUP_SHIFT_LARGE
#define ILCC_GROUP_SHIFT_LARGE 1   // config 5: 1: 90.4-90.8, 2: 87.1-88.1
#endif
constexpr int kGroupShiftSmall = ILCC_GROUP_SHIFT_SMALL, kGroupShiftLarge = ILCC_GROUP_SHIFT_LARGE;
template <int THREADS>
constexpr int kGroupShiftOf = kIsLargeInstance<THREADS> ? kGroupShiftLarge : kGroupShiftSmall;
constexpr int kBoxFirstRound = 32;                 // box pre-pass: points of the first round (an eighth of the sample, at least this many) when many tiles are alive ...
constexpr int kBoxFirstRoundFrom = 8;              // ... = from this many tiles per wavefront on (8 lanes or fewer per tile)
// box pre-pass: tile ids per compaction round = the length of the list of live tiles in LDS, a multiple of the workgroup size (the
// 256-thread instance: 512 B -- with 1 792 staged points a workgroup then needs 22.9 KB and SEVEN fit a CU's 160 KB)
template <int THREADS>
constexpr int kBoxSegment = THREADS <= 256 ? 256 : 1024;
constexpr int kBoxTilesMax = 4096;                 // box pre-pass: tiles per workgroup its LDS bit mask holds
constexpr float kBoxSafety = 1.f - 0x1p-12f;
constexpr int kBoundRefresh = 256;                  // points between reloads of the frame's shared bound

// tiles along an axis of n candidates, and of an n_ty x n_tz table
__host__ __device__ constexpr int axis_tiles(int n) { return (n + kTile - 1) / kTile; }
__host__ __device__ constexpr int grid_tiles(int n_ty, int n_tz) { return axis_tiles(n_ty) * axis_tiles(n_tz); }

// Dynamic LDS of a full-pass workgroup (k6_grid_cost): [cap float2 rotated points][cap float 0.5 * white][n_ty floats][n_tz floats].
// The kernel carves through grid_lds; launch_grid_cost, the raised dynamic-LDS limit and the handle's two-workgroups-per-CU cap
// (ilcc_api.cpp) size through grid_lds_bytes.
struct GridLds {
  size_t hw, ay, az, bytes;   // byte offsets of the parts behind the points, and the total
};
__host__ __device__ constexpr GridLds grid_lds(uint32_t cap, int n_ty, int n_tz) {
  GridLds l{};
  l.hw = sizeof(float2) * (size_t)cap;
  l.ay = l.hw + sizeof(float) * (size_t)cap;
  l.az = l.ay + sizeof(float) * (size_t)n_ty;
  l.bytes = l.az + sizeof(float) * (size_t)n_tz;
  return l;
}
__host__ __device__ constexpr size_t grid_lds_bytes(uint32_t cap, int n_ty, int n_tz) { return grid_lds(cap, n_ty, n_tz).bytes; }
// A kernel's carve: the part at byte offset `at` of a layout, reached from the part at `from_at` in steps of that part's elements
// (pointers made in the kernel from offsets: a carve that returned pointers, or added byte offsets to the base, compiled the
// full pass to another schedule)
template <class T, class U>
__device__ __forceinline__ T* lds_next(U* from, size_t from_at, size_t at) {
  return reinterpret_cast<T*>(from + (at - from_at) / sizeof(U));
}

// Dynamic LDS of a common pre-pass workgroup (k6_group_prepass): the widened pre-pass points (float4: at most M >> kGroupShift <= M / 2
// of the frame's M labelled points -- frames above grid_lds_points are clamped to this -- or box_points of them when that is more),
// then the (ty, tz) tables
static_assert(kGroupShiftSmall >= 1 && kGroupShiftLarge >= 1, "k6_group_prepass stages M >> kGroupShift <= M / 2 points: group_prepass_points holds that many");
__host__ __device__ constexpr uint32_t group_prepass_points(uint32_t grid_lds_points, uint32_t box_points) {
  return grid_lds_points / 2u + 64u > box_points ? grid_lds_points / 2u + 64u : box_points;
}
__host__ __device__ constexpr size_t group_prepass_lds_bytes(uint32_t grid_lds_points, uint32_t box_points, int n_ty, int n_tz) {
  return sizeof(float4) * (size_t)group_prepass_points(grid_lds_points, box_points) + sizeof(float) * (size_t)(n_ty + n_tz);
}

// the own box pre-pass's sample of a frame with Mfull labelled points, M of them walked by this launch, Mi of those interior class:
// Mfull >> shift border-class points (the frame's bound grows with its point count: so must the sample that has to exceed it), at
// least box_points, at most all of them
__device__ __forceinline__ uint32_t box_sample(uint32_t box_points, uint32_t Mfull, uint32_t M, uint32_t Mi, int shift) {
  return min(max(box_points, Mfull >> shift), M - Mi);
}

// the K6 kernels that stage a frame in dynamic LDS may use more than the 64 KiB default: up to the largest full-pass layout
// (params_ok bounds n_ty + n_tz by kGridTableMax).  One call per file that has such kernels, all from set_kernel_attributes_k6
inline hipError_t raise_grid_lds_limit(std::initializer_list<const void*> fns) {
  for (const void* fn : fns) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)grid_lds_bytes(kGridLdsPointsMax, kGridTableMax, 0));
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
hipError_t set_kernel_attributes_k6_group_prepass();
hipError_t set_kernel_attributes_k6_locate();

// sum over the 4 lanes of a quad (every lane gets the total): two DPP adds
__device__ __forceinline__ float quad_sum(float v) {
  v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0xB1 /*quad_perm [1,0,3,2]*/, 0xf, 0xf, false));
  v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x4E /*quad_perm [2,3,0,1]*/, 0xf, 0xf, false));
  return v;
}

// sum over aligned groups of P lanes (P a power of two, 2 ... 64; wave-uniform): every lane of a group gets the same bits (each
// step adds two values that both partners hold: a + b == b + a)
__device__ __forceinline__ float lanes_sum(float v, uint32_t P) {
  v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0xB1 /*quad_perm [1,0,3,2]*/, 0xf, 0xf, false));
  if (P > 2u) v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x4E /*quad_perm [2,3,0,1]*/, 0xf, 0xf, false));
  if (P > 4u) v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x141 /*row_half_mirror*/, 0xf, 0xf, false));
  if (P > 8u) v += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x140 /*row_mirror*/, 0xf, 0xf, false));
  if (P > 16u) v += __shfl_xor(v, 16);
  if (P > 32u) v += __shfl_xor(v, 32);
  return v;
}

struct Best {
  float cost;
  uint32_t d2;
  uint32_t flat;
};
__device__ __forceinline__ bool better(float c, uint32_t d2, uint32_t flat, const Best& b) {
  return c < b.cost || (c == b.cost && (d2 < b.d2 || (d2 == b.d2 && flat < b.flat)));
}

// argmin over the lanes of the wavefront (valid in lane 0); AB: carry each lane's (a << 16) | b along
template <bool AB>
__device__ __forceinline__ Best wave_argmin(Best best, uint32_t& ab) {
#pragma unroll
  for (int o = ILCC_WAVE / 2; o > 0; o >>= 1) {
    Best t;
    t.cost = __shfl_down(best.cost, o, ILCC_WAVE);
    t.d2 = __shfl_down(best.d2, o, ILCC_WAVE);
    t.flat = __shfl_down(best.flat, o, ILCC_WAVE);
    const uint32_t tab = AB ? __shfl_down(ab, o, ILCC_WAVE) : 0u;
    if (better(t.cost, t.d2, t.flat, best)) {
      best = t;
      if (AB) ab = tab;
    }
  }
  return best;
}
__device__ __forceinline__ Best wave_argmin(Best best) {
  uint32_t none = 0;
  return wave_argmin<false>(best, none);
}

// the workgroup's argmin over the wavefronts' bests its lanes 0 stored in LDS (read behind the barrier that follows the stores),
// ties to the lower wavefront; s_ab (optional): the wavefronts' (a << 16) | b, the winner's into ab
template <int WAVES>
__device__ __forceinline__ Best block_argmin(const Best* s_best, const uint32_t* s_ab, uint32_t& ab) {
  Best b = s_best[0];
  if (s_ab) ab = s_ab[0];
  for (int w = 1; w < WAVES; ++w)
    if (better(s_best[w].cost, s_best[w].d2, s_best[w].flat, b)) {
      b = s_best[w];
      if (s_ab) ab = s_ab[w];
    }
  return b;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = ILCC_WAVE / 2; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, ILCC_WAVE));
  return v;
}

// a completed candidate (theta k, translation (ia, ib)) of a launch's tables (n_ty x n_tz, entries nearest zero (c_th, c_ty, c_tz)) with
// the costs c0 / c1 of its two colour phases: into this lane's best (flat = 2 cell + phase) and its (ia << 16) | ib
__device__ __forceinline__ void score(float c0, float c1, int k, int ia, int ib, int n_ty, int n_tz, int c_th, int c_ty, int c_tz, Best& best,
                                      uint32_t& ab) {
  const uint32_t cell = ((uint32_t)k * (uint32_t)n_ty + (uint32_t)ia) * (uint32_t)n_tz + (uint32_t)ib;
  const uint32_t d2 = (uint32_t)((k - c_th) * (k - c_th) + (ia - c_ty) * (ia - c_ty) + (ib - c_tz) * (ib - c_tz));
  const uint32_t cab = ((uint32_t)ia << 16) | (uint32_t)ib;
  if (better(c0, d2, 2u * cell, best)) {
    best = Best{c0, d2, 2u * cell};
    ab = cab;
  }
  if (better(c1, d2, 2u * cell + 1u, best)) {
    best = Best{c1, d2, 2u * cell + 1u};
    ab = cab;
  }
}

// the record of a workgroup (or frame) that has no candidate at all
__device__ __forceinline__ void no_candidate(GridPartial* out) { *out = GridPartial{__builtin_inff(), 0xFFFFFFFFu, 0xFFFFFFFFu, 0u}; }

// Ctx::grid_iters: kIterSlots words per counter, frame f adds to word f mod kIterSlots of each (spread: fewer colliding atomics)
enum EvalCounter { kEvalsAll = 0, kEvalsInterior = 1, kEvalsBox = 2 };
__device__ __forceinline__ void count_evals(unsigned long long* grid_iters, uint32_t f, EvalCounter which, unsigned long long n) {
  atomicAdd(grid_iters + (int)which * kIterSlots + (f & (kIterSlots - 1)), n);
}

// first candidate of a window of `width` candidates that starts `before` candidates ahead of `centre`, kept inside an axis of n
__device__ __forceinline__ int window_origin(int centre, int before, int n, int width) {
  return min(max(centre - before, 0), max(n - width, 0));
}

// Rx(theta) on (0, y, z), already divided by g (Optimization.h:37-46).  Every launch rotates its points with this expression, which
// is what keeps the sums of the different launches of a frame bit for bit the same
// the walk prefix a subsampled (locate) launch looks at: M >> kSeedShift of the M positions, at least at_least
__device__ __forceinline__ uint32_t walk_sample(uint32_t M, uint32_t at_least) { return min(M, max(at_least, M >> kSeedShift)); }
// A sample of Ms of the M walk positions takes a proportional prefix of each part of the layout: n_in interior, n_rm rim, the rest
// other border-class points
__device__ __forceinline__ void walk_prefix(uint32_t Ms, uint32_t M, uint32_t Mi_all, uint32_t n_rim_all, uint32_t& n_in, uint32_t& n_rm) {
  n_in = Mi_all;
  n_rm = n_rim_all;
  if (Ms < M) {
    n_in = (uint32_t)(((uint64_t)Mi_all * Ms) / M);
    n_rm = (uint32_t)(((uint64_t)n_rim_all * Ms) / M);
  }
}
// walk position sl of that sample -> index in the walk layout.  (floor() twice in walk_prefix: the rest can be two positions longer
// than the other border-class part, hence the clamp)
__device__ __forceinline__ uint32_t layout_source(uint32_t sl, uint32_t n_in, uint32_t n_rm, uint32_t M, uint32_t Mi_all, uint32_t n_rim_all) {
  const uint32_t src = sl < n_in ? sl : sl < n_in + n_rm ? Mi_all + (sl - n_in) : Mi_all + n_rim_all + (sl - n_in - n_rm);
  return min(src, M - 1u);
}
// The frame's labelled points in walk order (k6_locate, k6_anchor).  With a walk layout (k5w_walk_order: every frame of at
// most kGridLdsPointsMax points) the layout is [interior class | rim | other border-class points], each part in golden-ratio order;
// without one, walk position s is point (s * S) mod M of the frame's own arrays.  (grid_cost_body calls the three functions above
// on fields of its own: held in a FrameWalk, they gave the full pass another register allocation and schedule.)
struct FrameWalk {
  const float2* __restrict__ yz;
  const uint8_t* __restrict__ lab;
  uint32_t M, S, Mi_all, n_rim_all;   // labelled points, golden-ratio stride, interior / rim class sizes of the layout
  bool layout;
  __device__ __forceinline__ FrameWalk(const Ctx& c, uint32_t f) : M(c.n_lab[f]), layout(M <= (uint32_t)kGridLdsPointsMax) {
    const uint64_t beg = c.off[f];
    yz = (layout ? c.walk_yz : c.yz) + beg;
    lab = (layout ? c.walk_lab : c.lab) + beg;
    S = (!layout && M) ? c.walk_stride[f] : 1u;
    Mi_all = layout ? c.walk_mi[f] : 0u;
    n_rim_all = layout ? c.walk_nrim[f] : 0u;
  }
  __device__ __forceinline__ uint32_t sample(uint32_t at_least) const { return walk_sample(M, at_least); }
  __device__ __forceinline__ void prefix(uint32_t Ms, uint32_t& n_in, uint32_t& n_rm) const { walk_prefix(Ms, M, Mi_all, n_rim_all, n_in, n_rm); }
  __device__ __forceinline__ uint32_t source(uint32_t sl, uint32_t n_in, uint32_t n_rm) const {
    return layout ? layout_source(sl, n_in, n_rm, M, Mi_all, n_rim_all) : (uint32_t)(((uint64_t)sl * S) % M);
  }
};

struct PointTerms {   // uniform across the wavefront
  float pi, pj, hw;   // rotated coordinates / g, and 0.5 * (label == white)
};

// one point under this lane's translation: adds cost / 2 to (A0, A1)
template <bool OOB>
__device__ __forceinline__ void accumulate(const PointTerms& p, float ay, float az, float Wh, float Hh, float delta,
                                           float& A0, float& A1) {
  const float i = p.pi + ay, j = p.pj + az;
  const float fi = floorf(i), fj = floorf(j);
  const float ai = (i - fi) - 0.5f, aj = (j - fj) - 0.5f;       // dist to the nearest integer = 0.5 - |a|
  const float Rin = 1.f - (fabsf(ai) + fabsf(aj));              // dist_i + dist_j
  const float mf = __builtin_amdgcn_fractf(fmaf(0.5f, fi + fj, p.hw));   // 0.5 iff (floor i + floor j + white) odd
  const float nmf = 0.5f - mf;
  const float ui = fabsf(i - Wh) - Wh, uj = fabsf(j - Hh) - Hh; // < 0 inside; |.| = min(|i|, |i-W|)
  const bool oob = fmaxf(ui, uj) >= 0.f;                         // not (0 < i < W and 0 < j < H)
  auto sel = [&](float if_oob, float otherwise) -> float { return oob ? if_oob : otherwise; };
  float R, w0, w1;
  if (OOB) {
    R = sel(fabsf(ui) + fabsf(uj), Rin);
    w0 = sel(0.5f, mf);
    w1 = sel(0.5f, nmf);
  } else {
    R = sel(0.f, Rin);
    w0 = mf;
    w1 = nmf;
  }
  const float Q = fminf(R, delta);
  const float T = Q * fmaf(-0.5f, Q, R);    // q (r - q/2) = 1/2 rho(r^2)
  A0 = fmaf(T, w0, A0);                     // += cost / 2 under topleftWhite = false
  A1 = fmaf(T, w1, A1);
}

// The same term for a point that is IN the board under every translation of this workgroup's tables (see the staging
// below): the out-of-board half of accumulate<> -- 10 of its 27.5 instructions -- is dead for it.  Same operations on
// the in-board side, so the value is bit-identical to what accumulate<> computes for such a point.
__device__ __forceinline__ void accumulate_interior(const PointTerms& p, float ay, float az, float delta, float& A0, float& A1) {
  const float i = p.pi + ay, j = p.pj + az;
  const float fi = floorf(i), fj = floorf(j);
  const float ai = (i - fi) - 0.5f, aj = (j - fj) - 0.5f;
  const float R = 1.f - (fabsf(ai) + fabsf(aj));
  const float mf = __builtin_amdgcn_fractf(fmaf(0.5f, fi + fj, p.hw));
  const float nmf = 0.5f - mf;
  const float Q = fminf(R, delta);
  const float T = Q * fmaf(-0.5f, Q, R);
  A0 = fmaf(T, mf, A0);
  A1 = fmaf(T, nmf, A1);
}


// Box pre-pass, one point against one tile: adds to lb a lower bound of the point's term (cost / 2, either colour phase) for
// EVERY translation in [alo, ahi] x [zlo, zhi] -- see the pre-pass in grid_cost_body for the argument.
// (pi_lo, pi_hi), (pj_lo, pj_hi): the point's rotated coordinates -- one value each (lo == hi) in a workgroup's own pre-pass, the
// extremes over the thetas of a group in k6_group_prepass's common pre-pass (fl(p + a) is monotone in p as in a).
__device__ __forceinline__ void box_term(float pi_lo, float pi_hi, float pj_lo, float pj_hi, float alo, float ahi, float zlo, float zhi,
                                         float Wh, float Hh, float delta, float& lb, bool count = true) {
  const float i_lo = pi_lo + alo, i_hi = pi_hi + ahi, j_lo = pj_lo + zlo, j_hi = pj_hi + zhi;
  const float ui_lo = fabsf(i_lo - Wh) - Wh, ui_hi = fabsf(i_hi - Wh) - Wh;
  const float uj_lo = fabsf(j_lo - Hh) - Hh, uj_hi = fabsf(j_hi - Hh) - Hh;
  const bool out_all = fmaxf(fminf(ui_lo, ui_hi), fminf(uj_lo, uj_hi)) >= 0.f;   // out of the board everywhere in the box
  // |u| closest to zero over the box: the end value nearer to zero, 0 when the ends differ in sign
  const float R = fabsf(__builtin_amdgcn_fmed3f(ui_lo, ui_hi, 0.f)) + fabsf(__builtin_amdgcn_fmed3f(uj_lo, uj_hi, 0.f));
  const float Q = fminf(R, delta);
  const float T = Q * fmaf(-0.5f, Q, R);
  lb = (out_all && count) ? fmaf(T, 0.5f, lb) : lb;   // (count = false: a lane past the end of the sample, evaluated branch-free)
}

// the best candidate of frame f among the records of the launch before, and the workgroup (seed launch: = seed theta index) that found it; wave-uniform.
// A handful of records: every lane reads them all (uniform addresses, scalar-cache loads) -- no cross-lane reduction.
__device__ __forceinline__ Best seed_argmin(const GridSeed& seed, uint32_t f, uint32_t& k2, uint32_t& ab) {
  const GridPartial* sp = seed.records + (uint64_t)f * seed.blocks;
  Best sb{__builtin_inff(), 0xFFFFFFFFu, 0xFFFFFFFFu};
  k2 = 0;
  ab = 0;
  for (uint32_t q = 0; q < seed.blocks; ++q) {
    const GridPartial g = sp[q];
    if (better(g.cost, g.d2, g.flat, sb)) {
      sb = Best{g.cost, g.d2, g.flat};
      k2 = q;       // seed launch: workgroup q = seed theta q
      ab = g.pad;   // (a << 16) | b of the record's candidate in ITS launch's tables
    }
  }
  return sb;
}

// Box pre-pass of one workgroup over the tiles whose bit in s_dead is clear (grid_cost_body's own pre-pass behind the common one's
// mask; k6_group_prepass over all tiles).  Round 5: the live tiles are COMPACTED into a list and the workgroup's lanes dealt out
// over them -- P lanes per tile (a power of two, 2 ... 64), each on every P-th point of the sample -- so that all lanes work on
// tiles that still need work; and when many tiles are alive a first round on the sample's first kBoxFirstRound points weeds out
// the tiles far from the minimum (most of them) before the survivors get the whole sample.  Segments of kBoxSegment<THREADS> tile ids keep
// the list small.  A tile's bound is a sum in an order that depends on P: kBoxSafety covers that (it is a lower bound in real
// arithmetic whatever the order; see box_term).  Sets the tile's bit in s_dead when its bound exceeds lim_box; *s_alive = 1 when
// a tile survives the whole sample.  cnt: two counters used in turn.  interval(u): the u-th point's (i_lo, i_hi, j_lo, j_hi).
// Returns the (point, tile) evaluations this wavefront really did (wave-uniform).  Ends with every thread past its last barrier
// -- the caller synchronises before it reads s_dead / *s_alive.
template <int THREADS, class Interval>
__device__ __forceinline__ uint32_t box_prepass_rounds(int n_tiles, int ntb, int a_org, int b_org, int n_ty, int n_tz, const float* s_ay,
                                                       const float* s_az, uint32_t* s_dead, uint16_t* s_live, uint32_t* cnt, uint32_t* s_alive,
                                                       uint32_t n_pre, float lim_box, float Wh, float Hh, float delta2, Interval interval) {
  constexpr int kWaves = THREADS / ILCC_WAVE;
  const int lane = lane_id();
  const int wid = __builtin_amdgcn_readfirstlane(wave_id());
  uint32_t wave_evals = 0, turn = 0;
  for (int seg0 = 0; seg0 < n_tiles; seg0 += kBoxSegment<THREADS>) {
    for (int round = 0; round < 2; ++round) {
      uint32_t* n_live = &cnt[turn & 1u];   // (two counters in turn: the next compaction's reset cannot overtake this one's readers)
      ++turn;
      if (threadIdx.x == 0) *n_live = 0u;
      __syncthreads();   // (also: s_dead initialised / the previous round's bits set; the previous list no longer read)
      for (int q = seg0 + (int)threadIdx.x; q < min(seg0 + kBoxSegment<THREADS>, n_tiles); q += THREADS) {   // (the segment is a multiple of THREADS: whole wavefronts)
        const bool live = !((s_dead[q >> 5] >> (q & 31)) & 1u);
        const unsigned long long m = __ballot(live);
        uint32_t base = 0;
        if (lane == 0 && m != 0ull) base = atomicAdd(n_live, (uint32_t)__popcll(m));
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (live) s_live[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)q;
      }
      __syncthreads();
      const uint32_t L = *n_live;   // live tiles of this segment (any order: a tile's sum does not depend on its place in the list)
      if (L == 0u) break;
      // tiles per wavefront: the smallest power of two that deals all L out in one go, at most 32 (P >= 2 lanes per tile)
      uint32_t tpw = 1u;
      while (tpw < 32u && tpw * (uint32_t)kWaves < L) tpw <<= 1;
      const uint32_t P = 64u / tpw, lgP = (uint32_t)__builtin_ctz(P);
      const uint32_t chk = min(8u, max(2u, 32u / P));   // points per lane between two looks at "is every tile of this wavefront beaten already"
      // many tiles alive: a first round on a prefix of the sample; few: the whole sample at once
      const uint32_t n_first = max((uint32_t)kBoxFirstRound, n_pre >> 3);
      const bool first = round == 0 && tpw >= (uint32_t)kBoxFirstRoundFrom && n_pre > 2u * n_first;
      const uint32_t n_use = first ? n_first : n_pre;
      const uint32_t slice = (uint32_t)lane & (P - 1u);
      for (uint32_t j0 = (uint32_t)wid * tpw; j0 < L; j0 += (uint32_t)kWaves * tpw) {
        const uint32_t j = j0 + ((uint32_t)lane >> lgP);
        const bool todo = j < L;
        const int q = (int)s_live[todo ? j : 0u];
        const int qa = q / ntb, qb = q - qa * ntb;
        float alo = __builtin_inff(), ahi = -__builtin_inff(), zlo = __builtin_inff(), zhi = -__builtin_inff();
#pragma unroll
        for (int d = 0; d < kTile; ++d) {
          const float va = s_ay[min(a_org + qa * kTile + d, n_ty - 1)], vz = s_az[min(b_org + qb * kTile + d, n_tz - 1)];
          alo = fminf(alo, va);
          ahi = fmaxf(ahi, va);
          zlo = fminf(zlo, vz);
          zhi = fmaxf(zhi, vz);
        }
        // (the sum only grows: a wavefront whose tiles are all beaten already stops looking at further points)
        float lb = 0.f, both = 0.f;
        const uint32_t wave_tiles = (uint32_t)__popcll(__ballot(todo && slice == 0u));
        for (uint32_t u0 = 0; u0 < n_use; u0 += P * chk) {
          wave_evals += wave_tiles * min(P * chk, n_use - u0);
          auto block = [&](auto n) {   // unrolled and branch-free, the LDS reads of four points issued together
            constexpr int N = decltype(n)::value, SUB = N >= 4 ? 4 : N;
#pragma unroll
            for (int d0 = 0; d0 < N; d0 += SUB) {
              float4 v[SUB];
              bool ok[SUB];
#pragma unroll
              for (int e = 0; e < SUB; ++e) {
                const uint32_t u = u0 + (uint32_t)(d0 + e) * P + slice;
                ok[e] = u < n_use && todo;
                v[e] = interval(min(u, n_use - 1u));
              }
#pragma unroll
              for (int e = 0; e < SUB; ++e) box_term(v[e].x, v[e].y, v[e].z, v[e].w, alo, ahi, zlo, zhi, Wh, Hh, delta2, lb, ok[e]);
            }
          };
          if (chk == 8u)
            block(std::integral_constant<int, 8>{});
          else if (chk == 4u)
            block(std::integral_constant<int, 4>{});
          else
            block(std::integral_constant<int, 2>{});
          both = lanes_sum(lb, P);   // the same bits in all P lanes of a tile
          if (__ballot(todo && !(both * kBoxSafety > lim_box)) == 0ull) break;
        }
        if (slice == 0u && todo) {
          if (both * kBoxSafety > lim_box)
            atomicOr(&s_dead[q >> 5], 1u << (q & 31));   // (a tile's bit is only ever set by its own lanes)
          else if (!first)
            *s_alive = 1u;
        }
      }
      if (!first) break;   // (uniform: first depends on L only)
    }
  }
  return wave_evals;
}

}  // namespace ilcc
