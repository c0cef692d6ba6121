// K7b corners: picks the phase with the lower with-OOB cost among the frame's solve records (K7a writes one or two, K7r
//      one), then builds the corner lattice:
//      LidarCornersEst::getPCDcorners (:501-556) with
//      transf = pcl::getTransformation(0, ty, tz, theta, 0, 0) (:412), and the display cloud
//      m_cloud_optim (:413).
#include "ilcc_internal.h"

namespace ilcc {

__device__ __forceinline__ void inv_rigid_apply(const float* T, const float in[3], float out[3]) {
  const float dx = in[0] - T[3], dy = in[1] - T[7], dz = in[2] - T[11];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float s = T[0 + c] * dx;
    s = s + T[4 + c] * dy;
    s = s + T[8 + c] * dz;
    out[c] = s;
  }
}

__global__ __launch_bounds__(kSolveThreads) void k7b_corners(Ctx c, const SolveRec* rec, int n_slots) {
  __shared__ float s_T[16];
  __shared__ uint32_t s_hit[kCoverageCellsMax / 32];
  __shared__ uint32_t s_oob;
  const uint32_t f = blockIdx.x;
  ilcc_result* r = &c.res[f];
  if (r->status != ILCC_OK) return;
  const uint32_t tid = threadIdx.x;
  const uint64_t beg = c.off[f];
  // phase selection: lower with-OOB cost, ties -> phase 0 (the reference's first hypothesis)
  SolveRec best = rec[2 * f];
  if (n_slots > 1) {
    const SolveRec o = rec[2 * f + 1];
    if (o.valid && (!best.valid || o.sel < best.sel)) best = o;
  }
  if (!best.valid) {
    if (tid == 0) r->status = ILCC_BAD_ARGUMENT;
    return;
  }
  // transf = pcl::getTransformation(0, ty, tz, theta, 0, 0): float Affine3f (:412)
  if (tid == 0) {
    r->theta_t[0] = best.x[0];
    r->theta_t[1] = best.x[1];
    r->theta_t[2] = best.x[2];
    r->cost_a = best.cost_a;
    r->cost_b = best.cost_b;
    r->sel_cost = best.sel;
    r->phase = best.phase;
    r->iters_a = best.iters_a;
    r->iters_b = best.iters_b;
    r->basin_margin = best.margin;
    r->flags = best.flags;
    r->grid_ties = best.ties;
    const float roll = (float)best.x[0];
    const float E = cosf(roll), F = sinf(roll);
    const float T[16] = {1, 0, 0, 0, 0, E, -F, (float)best.x[1], 0, F, E, (float)best.x[2], 0, 0, 0, 1};
    for (int k = 0; k < 16; ++k) s_T[k] = T[k];
    s_oob = 0u;
  }
  for (int k = (int)tid; k < kCoverageCellsMax / 32; k += kSolveThreads) s_hit[k] = 0u;
  __syncthreads();

  const int W = c.p.board_w, H = c.p.board_h;
  // Coverage of the virtual board by the labelled points (orc_coverage): the functor's own coordinates
  // (Optimization.h:37-49) in double.  What the operator checks at the viewer before pressing 'o' (:415-441).
  {
    const double g = c.p.grid_length, ct = cos(best.x[0]), st = sin(best.x[0]);
    const uint32_t nl = c.n_lab[f];
    const float2* __restrict__ yz = c.yz + beg;
    uint32_t oob = 0;
    for (uint32_t k = tid; k < nl; k += kSolveThreads) {
      const float2 v = yz[k];
      const double yy = ct * (double)v.x - st * (double)v.y + best.x[1];
      const double zz = st * (double)v.x + ct * (double)v.y + best.x[2];
      const double i = (yy + W * g / 2.0) / g, j = (zz + H * g / 2.0) / g;
      if (i > 0.0 && i < (double)W && j > 0.0 && j < (double)H) {
        const int cell = (int)floor(i) * H + (int)floor(j);
        atomicOr(&s_hit[cell >> 5], 1u << (cell & 31));
      } else {
        ++oob;
      }
    }
    if (oob) atomicAdd(&s_oob, oob);
    __syncthreads();
    if (tid == 0) {
      int cells = 0;
      for (int k = 0; k < (W * H + 31) / 32; ++k) cells += __popc(s_hit[k]);
      r->cells_hit = cells;
      r->n_oob = (int32_t)s_oob;
      if (c.p.min_cell_coverage > 0.0 && (double)cells < c.p.min_cell_coverage * (double)(W * H)) r->flags = best.flags | ILCC_FLAG_LOW_COVERAGE;
    }
  }
  const int nc = (W - 1) * (H - 1);
  const int ncc = nc < ILCC_MAX_CORNERS ? nc : ILCC_MAX_CORNERS;
  for (int t = (int)tid; t < ncc; t += kSolveThreads) {
    const int i = 1 + t / (H - 1), j = 1 + t % (H - 1);          // :513-534
    const double xg = (i - (double)W / 2.0) * c.p.grid_length;
    const double yg = (j - (double)H / 2.0) * c.p.grid_length;
    const float pt[3] = {0.0f, (float)xg, (float)yg};
    float a[3], w[3];
    inv_rigid_apply(s_T, pt, a);        // transOptim.inverse() :548
    inv_rigid_apply(r->pca, a, w);      // transPCA.inverse()   :549
    r->corners[3 * t] = w[0];
    r->corners[3 * t + 1] = w[1];
    r->corners[3 * t + 2] = w[2];
  }
  if (tid == 0) r->n_corners = ncc;

  // m_cloud_optim = transf * m_cloud_PCA (:413), float
  const uint32_t M = (uint32_t)r->n_plane;
  const float4* __restrict__ Q = c.pca + beg;
  float4* __restrict__ O = c.optim + beg;
  for (uint32_t i = tid; i < M; i += kSolveThreads) {
    const float4 v = Q[i];
    float o[3];
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
      float s = s_T[4 * rr] * v.x;
      s = s + s_T[4 * rr + 1] * v.y;
      s = s + s_T[4 * rr + 2] * v.z;
      s = s + s_T[4 * rr + 3];
      o[rr] = s;
    }
    O[i] = make_float4(o[0], o[1], o[2], v.w);
  }
  // GRID mode: a neighbouring basin that costs (almost) the same -> the caller is told (corners stay in the record).
  // Written last: every thread above read r->status == ILCC_OK before this store can land (barrier)
  __syncthreads();
  if (tid == 0 && c.p.solver == ILCC_SOLVER_GRID && c.p.ambiguity_eps > 0.0 && best.margin < c.p.ambiguity_eps) r->status = ILCC_AMBIGUOUS;
}

void launch_corners(const Ctx& c, hipStream_t s, int n_slots) {
  hipLaunchKernelGGL(k7b_corners, dim3(c.n_frames), dim3(kSolveThreads), 0, s, c, c.solve_rec, n_slots);
}

}  // namespace ilcc
