// K5w -- the frame's labelled points in K6's walk layout (k5w_walk_order in k5w_walk_order.hip, k345_front_end in
// k345_front_end.hip).
#pragma once

#include "ilcc_internal.h"

namespace ilcc {

__device__ __forceinline__ float2 rotate(float2 v, float cth, float sth) {
  return make_float2(fmaf(-sth, v.y, cth * v.x), fmaf(cth, v.y, sth * v.x));
}

// K5w walk order: the frame's labelled points in the layout k6_grid_cost stages -- [interior | rim | other border], each part
// in golden-ratio walk order -- written ONCE per frame (round 3 until here: every one of a frame's ~80 K6 workgroups
// classified and partitioned the points again, 20 % of the full pass's VALU instructions).
//   interior: in the board under every rotation of the theta table and every translation of the (ty, tz) tables -- decided
//             by a bound, not by trying the 61 rotations (that loop was 10 M of the path's 386 M instructions per 512 frames
//             and found 7 % more points): |i| <= |y| max|cos| + |z| max|sin|, with a margin far above fp32 rounding; the
//             decimated tables of the seed launch are subsets of the full ones -> accumulate_interior is exact for these
//             points in every launch;
//   rim:      border-class and within kRimMilli thousandths of a square of the outline at the grid's centre candidate:
//             walked first, they are the points that leave the board when the translation is wrong (ordering only).
constexpr int kRimMilli = 300;   // rim = within 0.3 square of the outline
// One frame, by its workgroup of kWalkThreads threads.  The M labelled points come through `src` -- c.yz / c.lab, or a copy in LDS --
// and the class of walk slot sl is kept in s_cls[sl * cls_stride] (LDS, the caller's, as are the 3 * kWalkThreads / 64 words of
// s_cnt).  Nothing here can be contracted into an FMA that is not written as one (the only product that feeds a sum, 2 Wh, is
// exact), so the layout does not depend on the -ffp-contract setting of the file that includes this.
struct WalkSource {
  const float* yz;      // point i: y at yz[i * yz_stride], z one float behind it
  uint32_t yz_stride;
  const uint8_t* lab;   // point i: lab[i * lab_stride]
  uint32_t lab_stride;
};
__device__ __forceinline__ void walk_order_frame(const Ctx& c, const uint32_t f, const uint32_t M, const uint32_t S, const WalkSource src,
                                                 uint8_t* s_cls, const uint32_t cls_stride, uint32_t* s_cnt) {
  uint32_t *s_in = s_cnt, *s_rim = s_cnt + kWalkThreads / ILCC_WAVE, *s_oth = s_cnt + 2 * (kWalkThreads / ILCC_WAVE);
  if (M == 0u || M > (uint32_t)kGridLdsPointsMax) {   // K6 walks such a frame through global memory in golden-ratio order
    if (threadIdx.x == 0) {
      c.walk_mi[f] = 0u;
      c.walk_nrim[f] = 0u;
    }
    return;
  }
  const int lane = lane_id();
  const int wid = wave_id();
  const uint64_t beg = c.off[f];
  auto point = [&](uint32_t i) { return make_float2(src.yz[(size_t)i * src.yz_stride], src.yz[(size_t)i * src.yz_stride + 1]); };
  const float Wh = 0.5f * (float)c.p.board_w, Hh = 0.5f * (float)c.p.board_h;
  const GridTables& t = c.grid;
  const float ay_lo = t.ay[0], ay_hi = t.ay[t.n_ty - 1], az_lo = t.az[0], az_hi = t.az[t.n_tz - 1];
  const float ay_c = t.ay[t.c_ty], az_c = t.az[t.c_tz];
  const float rim_thr = -(float)kRimMilli * 1e-3f;
  const int n_th = t.n_th;
  float cmax = 0.f, smax = 0.f;   // (uniform: the tables are a few dozen values)
  for (int k = 0; k < n_th; ++k) {
    cmax = fmaxf(cmax, fabsf(t.cth[k]));
    smax = fmaxf(smax, fabsf(t.sth[k]));
  }
  const float room_i = fminf(fminf(ay_lo, ay_hi), 2.f * Wh - fmaxf(ay_lo, ay_hi)), room_j = fminf(fminf(az_lo, az_hi), 2.f * Hh - fmaxf(az_lo, az_hi));
  // class of every walk slot: 0 interior, 1 other border, 2 rim
  uint32_t cnt_in = 0, cnt_rim = 0;
  for (uint32_t sl = threadIdx.x; sl < M; sl += kWalkThreads) {
    const float2 v = point((uint32_t)(((uint64_t)sl * S) % M));
    // |i| <= |y| max|cos/g| + |z| max|sin/g| for every theta of the table (and likewise |j|): inside the room the translations
    // leave on both axes, with 1e-4 square to spare, the point is in the board for every candidate -- fp32 rounding of the
    // term's own expressions (a few 1e-7 on coordinates of a few squares) included
    const float bi = fmaf(fabsf(v.y), smax, fabsf(v.x) * cmax), bj = fmaf(fabsf(v.y), cmax, fabsf(v.x) * smax);
    const bool inside_always = bi + 1e-4f < room_i && bj + 1e-4f < room_j;
    int cl = 0;
    if (!inside_always) {
      const float2 p = rotate(v, t.cth[t.c_th], t.sth[t.c_th]);
      const float uc = fabsf((p.x + ay_c) - Wh) - Wh, wc = fabsf((p.y + az_c) - Hh) - Hh;
      cl = (fmaxf(uc, wc) > rim_thr) ? 2 : 1;
    }
    s_cls[(size_t)sl * cls_stride] = (uint8_t)cl;
    cnt_in += cl == 0;
    cnt_rim += cl == 2;
  }
  cnt_in = wave_sum(cnt_in);
  cnt_rim = wave_sum(cnt_rim);
  if (lane == 0) {
    s_in[wid] = cnt_in;
    s_rim[wid] = cnt_rim;
  }
  __syncthreads();
  uint32_t Mi = 0, n_rim = 0;
  for (int w = 0; w < kWalkThreads / ILCC_WAVE; ++w) {
    Mi += s_in[w];
    n_rim += s_rim[w];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    c.walk_mi[f] = Mi;
    c.walk_nrim[f] = n_rim;
  }
  // stable partition, chunk by chunk (ballot ranks inside a wavefront, counts of the wavefronts in LDS): deterministic
  float2* __restrict__ wyz = c.walk_yz + beg;
  uint8_t* __restrict__ wlab = c.walk_lab + beg;
  uint32_t base_in = 0, base_rim = Mi, base_oth = Mi + n_rim;
  for (uint32_t c0 = 0; c0 < M; c0 += kWalkThreads) {
    const uint32_t sl = c0 + threadIdx.x;
    const int cl = sl < M ? (int)s_cls[(size_t)sl * cls_stride] : -1;
    const unsigned long long m_in = __ballot(cl == 0), m_oth = __ballot(cl == 1), m_rim = __ballot(cl == 2);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (lane == 0) {
      s_in[wid] = (uint32_t)__popcll(m_in);
      s_rim[wid] = (uint32_t)__popcll(m_rim);
      s_oth[wid] = (uint32_t)__popcll(m_oth);
    }
    __syncthreads();
    uint32_t pre_in = 0, pre_rim = 0, pre_oth = 0, tot_in = 0, tot_rim = 0, tot_oth = 0;
    for (int w = 0; w < kWalkThreads / ILCC_WAVE; ++w) {
      const uint32_t a = s_in[w], r = s_rim[w], o = s_oth[w];
      if (w < wid) {
        pre_in += a;
        pre_rim += r;
        pre_oth += o;
      }
      tot_in += a;
      tot_rim += r;
      tot_oth += o;
    }
    if (cl >= 0) {
      const uint32_t at = cl == 0   ? base_in + pre_in + (uint32_t)__popcll(m_in & below)
                          : cl == 2 ? base_rim + pre_rim + (uint32_t)__popcll(m_rim & below)
                                    : base_oth + pre_oth + (uint32_t)__popcll(m_oth & below);
      const uint32_t i = (uint32_t)(((uint64_t)sl * S) % M);
      wyz[at] = point(i);
      wlab[at] = src.lab[(size_t)i * src.lab_stride];
    }
    base_in += tot_in;
    base_rim += tot_rim;
    base_oth += tot_oth;
    __syncthreads();
  }
}

}  // namespace ilcc
