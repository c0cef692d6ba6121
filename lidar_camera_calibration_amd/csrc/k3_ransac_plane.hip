// K3 ransac_plane -- replaces pcl::SACSegmentation (SACMODEL_PLANE, SAC_RANSAC, threshold
// 0.03 m, optimize coefficients) of LidarCornersEst::getPlane
// (/root/reference/ilcc2/src/LidarCornersEst.cpp:190-221).
//
// One workgroup per frame (4 wavefronts; 16 in small batches).  Each wavefront scores whole
// hypotheses: the three sample indices come from a counter-based hash (PCL's boost::mt19937
// stream cannot be reproduced without PCL), every lane strides over the cluster points and
// the inlier count (|n.p+d| < thr, strict, float, unfused) is reduced with ballot/popcount.
// How many hypotheses: PCL's own rule (RandomSampleConsensus: k = log(1 - p) / log(1 - w^3), round 5).
// Winner = most inliers, ties -> lowest hypothesis index.  Then PCL's refinement:
// PCA plane of the inliers (double accumulation, Jacobi eigen-solver) and re-selection of
// the inliers with the refined plane, emitted in input order (= m_cloud_chessboard).
//
// The stage itself is ransac_plane_frame (k3_ransac_plane.h), shared with the front end's one-launch kernel.
#include "k3_ransac_plane.h"

namespace ilcc {

__global__ __launch_bounds__(kPlaneThreadsSmallBatch) void k3_ransac_plane(Ctx c) {
  __shared__ float4 s_P[kRansacLdsPoints];
  __shared__ uint32_t sc[64];
  __shared__ double scd[16 * 6 + 8];
  const uint32_t f = blockIdx.x;
  if (c.res[f].status != ILCC_OK) return;
  uint32_t n_plane;
  bool staged;
  (void)ransac_plane_frame(c, f, s_P, sc, scd, /*keep_in_lds=*/false, n_plane, staged);
}

void launch_ransac_plane(const Ctx& c, hipStream_t s) {
  const int threads = (c.n_frames <= (uint32_t)kSmallBatchFrames || c.wide) ? kPlaneThreadsSmallBatch : kPlaneThreads;
  hipLaunchKernelGGL(k3_ransac_plane, dim3(c.n_frames), dim3(threads), 0, s, c);
}

}  // namespace ilcc
