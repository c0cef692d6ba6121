// K3 -> K4/K5 -> K5w in ONE launch: one workgroup of 256 threads per frame takes the frame from its cluster to its walk layout.
//
// A frame's plane fit, plane frame, labels and walk layout depend on that frame only, and in a batch of many frames the three
// kernels run at the same width.  As three launches each pays its own ramp, its own wait for wave slots beside another batch's K6
// full pass and its own tail (the batch waits for the slowest frame of EACH of them), and hands its points to the next through
// L2.  Here the cluster is staged in LDS once (K3's s_P) and stays there: the re-selected inliers are compacted in place, K4's
// passes and the histogram read them from LDS, the transformed points replace them in place, the labelled ones are compacted in
// place once more, and K5w's class pass and partition read those.  Everything the other stages and the fetch entries read is
// still written as before: board, pca, yz / lab / cls, the walk layout, the result record.
//
// The stages are the same functions the three kernels call (ransac_plane_frame, plane_frame_hist_frame, walk_order_frame), on the
// same 256 threads with the same index-to-thread map and block reductions: every double sum, hence every decision, is
// bit-identical to the three launches.  A cluster above kRansacLdsPoints keeps all three stages on their global-memory paths.
//
// LDS: K3's 32 KiB of staging, one sc / scd scratch lent to every stage, the stages' own few words and the histogram -- about
// 0.3 KiB + (hist_bins + 1) counters above K3 alone, four workgroups to a CU as before.  K5w's classes need no room of their own:
// with the points in LDS they sit in the unused fourth word of each point's slot, otherwise in the staging nobody uses.
#include "k3_ransac_plane.h"
#include "k45_plane_frame_hist.h"
#include "k5w_walk_order.h"

namespace ilcc {

constexpr int kFrontThreads = kPlaneThreads;
static_assert(kRansacLdsPoints * sizeof(float4) >= (size_t)kGridLdsPointsMax, "K5w's classes fit the unused staging");

__global__ __launch_bounds__(kFrontThreads) void k345_front_end(Ctx c, uint32_t walk_layout) {
  __shared__ float4 s_P[kRansacLdsPoints];
  __shared__ uint32_t sc[64];
  __shared__ double scd[16 * 6 + 8];
  extern __shared__ int s_hist[];   // hist_bins + 1 counters
  const uint32_t f = blockIdx.x;
  if (c.res[f].status != ILCC_OK) return;
  const uint64_t beg = c.off[f];
  uint32_t n_plane, n_lab, S;
  bool staged;
  if (!ransac_plane_frame(c, f, s_P, sc, scd, /*keep_in_lds=*/true, n_plane, staged)) return;
  // (two calls, not one on a selected pointer: each is compiled for the address space it reads)
  if (staged) {
    if (!plane_frame_hist_frame(c, f, s_P, n_plane, sc, scd, s_hist, s_P, n_lab, S) || !walk_layout) return;
    // a labelled point's slot: y, z, label bits, (free: the class of walk slot i)
    uint8_t* bytes = reinterpret_cast<uint8_t*>(s_P);
    walk_order_frame(c, f, n_lab, S, WalkSource{reinterpret_cast<const float*>(s_P), 4u, bytes + 8, 16u}, bytes + 12, 16u, sc);
  } else {
    if (!plane_frame_hist_frame(c, f, c.board + beg, n_plane, sc, scd, s_hist, nullptr, n_lab, S) || !walk_layout) return;
    walk_order_frame(c, f, n_lab, S, WalkSource{reinterpret_cast<const float*>(c.yz + beg), 2u, c.lab + beg, 1u},
                     reinterpret_cast<uint8_t*>(s_P), 1u, sc);
  }
}

void launch_front_end(const Ctx& c, hipStream_t s, bool walk_layout) {
  const size_t lds = sizeof(int) * (size_t)(c.p.hist_bins + 1);
  hipLaunchKernelGGL(k345_front_end, dim3(c.n_frames), dim3(kFrontThreads), lds, s, c, walk_layout ? 1u : 0u);
}

}  // namespace ilcc
