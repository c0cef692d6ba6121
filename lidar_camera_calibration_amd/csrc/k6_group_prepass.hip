// K6 common pre-pass: one box pre-pass per (frame, group of kThetaGroup thetas) in front of the full pass (k6_grid_cost.hip)
#include "k6_common.h"

namespace ilcc {

// k6_group_prepass: ONE box pre-pass for a GROUP of kThetaGroup consecutive thetas, in front of the full pass.  71 % of the (frame,
// theta) workgroups of the full pass die in their own box pre-pass -- staging, tables, three barriers, ~450 instructions per
// wavefront each: 30 % of the kernel -- and a theta step moves a point by less than a third of a tile's width.  Every pre-pass
// point is rotated by all thetas of the group (the term's own fp32 expressions) and the box bound takes the extremes: i_lo from the
// smallest rotated coordinate and the box's lowest translation, i_hi from the largest and the highest.  fl(p + a) is monotone
// in p as in a, so [i_lo, i_hi] contains the interval each theta's own pre-pass uses: the bound is a lower bound for all group x 16
// candidates by box_term's argument unchanged (a point whose images lie more than half a square apart on an axis is left
// out; the interval stays far narrower than a board).  Output per (frame, group): a state word -- 0: every tile rejected (the
// group's full-pass workgroups exit on their first instructions), 1: a bit mask of the rejected tiles follows (their own
// pre-pass starts from it and only looks at the rest), 2: no common pre-pass (conditions not met) -- and the mask.

// The hand-over to the full pass (GridPass::work_list; one thread of the pre-pass workgroup): a group with something left to do --
// state 1, or state 2 on a frame with status ILCC_OK -- lists its nk (frame, theta) workgroups; for every other group the pre-pass
// writes the nk records a full-pass workgroup would have written on its first instructions.  Either way the full pass's records
// are what the (n_th, F) launch alone leaves; the listed launch simply never starts the workgroups with nothing to do.
__device__ __forceinline__ void hand_over_group(const GridPass& pass, uint32_t f, int k0, int nk, bool live) {
  if (pass.work_list == nullptr) return;
  const uint32_t first = f * pass.blocks + (uint32_t)k0;
  if (live) {
    const uint32_t at = atomicAdd(pass.work_count, (uint32_t)nk);   // (at most n_frames x blocks items over the launch: the list's size)
    for (int t = 0; t < nk; ++t) pass.work_list[at + (uint32_t)t] = first + (uint32_t)t;
  } else {
    for (int t = 0; t < nk; ++t) no_candidate(&pass.out[first + (uint32_t)t]);
  }
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void k6_group_prepass(Ctx c, GridPass pass) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ uint32_t s_iters[THREADS / ILCC_WAVE];
  __shared__ uint32_t s_dead3[kBoxTilesMax / 32];
  __shared__ uint16_t s_live[kBoxSegment<THREADS>];   // the tiles still alive, compacted (box_prepass_rounds)
  __shared__ uint32_t s_cnt2[2];
  __shared__ uint32_t s_any;
  const uint32_t f = blockIdx.y;
  const int k0 = kThetaGroup * (int)blockIdx.x, nk = min(kThetaGroup, pass.t.n_th - k0);
  const uint32_t tr = f * pass.grp_count + blockIdx.x;
  const uint32_t Mall = c.n_lab[f];
  // (frames above the full pass's staging capacity have a walk layout too -- k5w lays out every frame of at most kGridLdsPointsMax
  // points -- and their full pass reads this mask in its OVERFLOW form)
  const bool lds = Mall <= (uint32_t)kGridLdsPointsMax;
  const int n_ty = pass.t.n_ty, n_tz = pass.t.n_tz;
  const int nta = axis_tiles(n_ty), ntb = axis_tiles(n_tz), n_tiles = nta * ntb;
  const uint32_t Mi = lds ? c.walk_mi[f] : 0u;
  // (every condition is uniform over the workgroup)
  const bool frame_ok = c.res[f].status == ILCC_OK;
  if (!(frame_ok && lds && nk > 1 && pass.box_points != 0u && n_tiles <= kBoxTilesMax && Mall > Mi)) {
    if (threadIdx.x == 0) {
      pass.grp_alive[tr] = 2u;
      hand_over_group(pass, f, k0, nk, frame_ok);   // (a frame that never reached the search: its full-pass workgroups only write no_candidate)
    }
    return;
  }
  const int lane = lane_id();
  const int wid = __builtin_amdgcn_readfirstlane(wave_id());
  // (the sample never exceeds what group_prepass_lds_bytes holds: any prefix of the rim-first walk gives a valid bound)
  const uint32_t n_pre = min(box_sample(pass.box_points, Mall, Mall, Mi, kGroupShiftOf<THREADS>), group_prepass_points(c.grid_lds_points, pass.box_points));
  float4* s_w4 = reinterpret_cast<float4*>(smem);   // n_pre x (pi_lo, pi_hi, pj_lo, pj_hi)
  float* s_ay = reinterpret_cast<float*>(s_w4 + n_pre);
  float* s_az = s_ay + n_ty;
  const float2* __restrict__ wyz = c.walk_yz + c.off[f];
  float cth[kThetaGroup], sth[kThetaGroup];
#pragma unroll
  for (int t = 0; t < kThetaGroup; ++t) {
    cth[t] = pass.t.cth[k0 + min(t, nk - 1)];
    sth[t] = pass.t.sth[k0 + min(t, nk - 1)];
  }
  for (uint32_t sl = threadIdx.x; sl < n_pre; sl += THREADS) {
    const float2 v = wyz[Mi + sl];   // the rim-first border-class part of the walk layout: what each theta's own pre-pass looks at
    float ilo = __builtin_inff(), ihi = -__builtin_inff(), jlo = __builtin_inff(), jhi = -__builtin_inff();
#pragma unroll
    for (int t = 0; t < kThetaGroup; ++t) {
      const float2 p = rotate(v, cth[t], sth[t]);
      ilo = fminf(ilo, p.x);
      ihi = fmaxf(ihi, p.x);
      jlo = fminf(jlo, p.y);
      jhi = fmaxf(jhi, p.y);
    }
    // a point far from the rotation centre: leave it out (as a point at the board's centre, in the board under every
    // translation of the tables -- the host launches this kernel only then -- it contributes nothing to any bound)
    const bool wide = !(ihi - ilo <= 0.5f && jhi - jlo <= 0.5f);
    s_w4[sl] = wide ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(ilo, ihi, jlo, jhi);
  }
  for (int i = threadIdx.x; i < n_ty; i += THREADS) s_ay[i] = pass.t.ay[i];
  for (int i = threadIdx.x; i < n_tz; i += THREADS) s_az[i] = pass.t.az[i];
  for (int w = threadIdx.x; w < (n_tiles + 31) / 32; w += THREADS) s_dead3[w] = 0u;
  if (threadIdx.x == 0) s_any = 0u;
  __syncthreads();
  const float Wh = 0.5f * (float)c.p.board_w, Hh = 0.5f * (float)c.p.board_h, delta2 = (float)c.p.huber_delta;
  const float lim_box = 0.5f * (1.f + kTieEps) * __uint_as_float(__hip_atomic_load(pass.bound + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  const uint32_t wave_evals = box_prepass_rounds<THREADS>(n_tiles, ntb, 0, 0, n_ty, n_tz, s_ay, s_az, s_dead3, s_live, s_cnt2, &s_any, n_pre, lim_box, Wh, Hh,
                                                          delta2, [&](uint32_t u) { return s_w4[u]; });
  if (lane == 0) s_iters[wid] = wave_evals;
  __syncthreads();
  const bool any_alive = s_any != 0u;
  if (any_alive)
    for (int w = threadIdx.x; w < (n_tiles + 31) / 32; w += THREADS) pass.grp_mask[(uint64_t)tr * pass.grp_words + w] = s_dead3[w];
  if (threadIdx.x == 0) {
    unsigned long long box_evals = 0;
    for (int w = 0; w < THREADS / ILCC_WAVE; ++w) box_evals += s_iters[w];
    count_evals(c.grid_iters, f, kEvalsBox, box_evals);
    pass.grp_alive[tr] = any_alive ? 1u : 0u;
    hand_over_group(pass, f, k0, nk, any_alive);
  }
}

void launch_group_prepass(const Ctx& c, const GridPass& full, hipStream_t s) {
  const dim3 grid(full.grp_count, c.n_frames);
  const size_t lds = group_prepass_lds_bytes(c.grid_lds_points, full.box_points, full.t.n_ty, full.t.n_tz);
  if (c.grid_lds_points > (uint32_t)kGridLargeFrom)
    hipLaunchKernelGGL((k6_group_prepass<kGridThreadsLarge>), grid, dim3(kGridThreadsLarge), lds, s, c, full);
  else
    hipLaunchKernelGGL((k6_group_prepass<kGridThreads>), grid, dim3(kGridThreads), lds, s, c, full);
}

hipError_t set_kernel_attributes_k6_group_prepass() {
  return raise_grid_lds_limit({(const void*)k6_group_prepass<kGridThreads>, (const void*)k6_group_prepass<kGridThreadsLarge>});
}

}  // namespace ilcc
