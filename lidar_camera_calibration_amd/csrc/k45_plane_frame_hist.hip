// K4 plane_frame + K5 gray_zone_hist, fused: one workgroup of kHistThreads (256) threads per frame.
//
// K4 replaces LidarCornersEst::transformbyPCA (/root/reference/ilcc2/src/LidarCornersEst.cpp:330-364):
//   compute3DCentroid, computeCovarianceMatrixNormalized (/N), SelfAdjointEigenSolver
//   (ascending), col(2) = col(0) x col(1), T = [E^T | -E^T c], transformPointCloud.
//   Accumulation is double (PCL: float); the eigenvector sign convention (Eigen: unspecified)
//   is: normal towards the sensor, e1's largest-magnitude component positive.
// K5 replaces calHist + get_gray_zone (:224-328) on the intensities of m_cloud_chessboard and
//   the black/gray/white classification of Optimization::get_theta_t
//   (/root/reference/ilcc2/src/Optimization.cpp:114-125); the non-gray points are written as a
//   compact (y,z) + label stream, the only thing the cost kernels read.
//
// The stage itself is plane_frame_hist_frame (k45_plane_frame_hist.h), shared with the front end's one-launch kernel.
#include "k45_plane_frame_hist.h"

namespace ilcc {

__global__ __launch_bounds__(kHistThreads) void k45_plane_frame_hist(Ctx c) {
  __shared__ uint32_t sc[64];
  __shared__ double scd[16 * 6 + 8];
  extern __shared__ int s_hist[];   // hist_bins + 1 counters
  const uint32_t f = blockIdx.x;
  if (c.res[f].status != ILCC_OK) return;
  const float4* __restrict__ P = c.board + c.off[f];
  uint32_t n_lab, S;
  (void)plane_frame_hist_frame(c, f, P, (uint32_t)c.res[f].n_plane, sc, scd, s_hist, nullptr, n_lab, S);
}

void launch_plane_frame_hist(const Ctx& c, hipStream_t s) {
  const size_t lds = sizeof(int) * (size_t)(c.p.hist_bins + 1);
  hipLaunchKernelGGL(k45_plane_frame_hist, dim3(c.n_frames), dim3(kHistThreads), lds, s, c);
}

}  // namespace ilcc
