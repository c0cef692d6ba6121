// k7_common.h -- what more than one of the K7 stage files needs: the register-only lane exchanges of the two solvers
// (k7a_local_solve.hip, k7r_pattern_refine.hip), the LDS layout of a frame's staged labelled points, and the number of
// phase slots a batch solves (K7a writes them, K7b reads them).  No stage bodies live here.
#pragma once

#include "ilcc_internal.h"

namespace ilcc {

// v[lane ^ MASK] for a 64-bit value, in registers only: v_permlane32_swap / v_permlane16_swap (gfx950) and
// DPP row rotations / quad permutes on the two dwords -- no ds_bpermute round trips.
template <int CTRL, int BANK = 0xf>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t old, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, 0xf, BANK, false);
}
template <int MASK>
__device__ __forceinline__ uint32_t xor_lane_u32(uint32_t v) {
  if constexpr (MASK == 32) {
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return (lane_id() & 32) ? r[0] : r[1];   // swap exchanges the upper half of operand 0 with the lower half of operand 1
  } else if constexpr (MASK == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return (lane_id() & 16) ? r[0] : r[1];
  } else if constexpr (MASK == 8) {
    return dpp_u32<0x128>(0u, v);                       // row_ror:8
  } else if constexpr (MASK == 4) {
    const uint32_t lo = dpp_u32<0x124, 0xa>(0u, v);     // row_ror:4 -> banks 1,3 take lane i-4
    return dpp_u32<0x12C, 0x5>(lo, v);                  // row_ror:12 -> banks 0,2 take lane i+4
  } else if constexpr (MASK == 2) {
    return dpp_u32<0x4E>(0u, v);                        // quad_perm [2,3,0,1]
  } else {
    return dpp_u32<0xB1>(0u, v);                        // quad_perm [1,0,3,2]
  }
}
template <int MASK>
__device__ __forceinline__ double xor_lane_f64(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const uint32_t lo = xor_lane_u32<MASK>((uint32_t)b), hi = xor_lane_u32<MASK>((uint32_t)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
template <int MASK>
__device__ __forceinline__ unsigned long long xor_lane_u64(unsigned long long b) {
  const uint32_t lo = xor_lane_u32<MASK>((uint32_t)b), hi = xor_lane_u32<MASK>((uint32_t)(b >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// The labelled points of `frames` frames staged in one workgroup's dynamic LDS, `cap` points each: every frame's float2
// block first, then every frame's label block, frame k at k * cap in each.  The kernels carve through staged_points and
// the host sizes launches and limits through staged_points_bytes, so the two cannot disagree.
struct StagedPoints {
  float2* yz;
  uint8_t* lab;
};
__host__ __device__ inline size_t staged_points_bytes(uint32_t cap, uint32_t frames) {
  return (sizeof(float2) + 1) * (size_t)cap * (size_t)frames;
}
__device__ __forceinline__ StagedPoints staged_points(unsigned char* smem, uint32_t cap, uint32_t frames, uint32_t k) {
  return StagedPoints{reinterpret_cast<float2*>(smem) + (size_t)k * cap,
                      smem + sizeof(float2) * (size_t)cap * (size_t)frames + (size_t)k * cap};
}

// solves per frame: both colour phases only where the reference solver is asked to try both
inline int solve_slots(const ilcc_params& p) { return (p.solver == ILCC_SOLVER_REFERENCE_LOCAL && p.phase_mode == 2) ? 2 : 1; }

}  // namespace ilcc
