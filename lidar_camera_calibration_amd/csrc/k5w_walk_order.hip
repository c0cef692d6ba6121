// K5w as a launch of its own (the front end's one-launch kernel, k345_front_end.hip, runs the same stage)
#include "k6_common.h"

namespace ilcc {

// K5w: the stage itself is walk_order_frame (k5w_walk_order.h), shared with the front end's one-launch kernel
__global__ __launch_bounds__(kWalkThreads) void k5w_walk_order(Ctx c) {
  __shared__ uint8_t s_cls[kGridLdsPointsMax];
  __shared__ uint32_t s_cnt[3 * (kWalkThreads / ILCC_WAVE)];
  const uint32_t f = blockIdx.x;
  if (c.res[f].status != ILCC_OK) return;
  const uint64_t beg = c.off[f];
  walk_order_frame(c, f, c.n_lab[f], c.walk_stride[f], WalkSource{reinterpret_cast<const float*>(c.yz + beg), 2u, c.lab + beg, 1u}, s_cls, 1u, s_cnt);
}

void launch_walk_order(const Ctx& c, hipStream_t s) {
  hipLaunchKernelGGL(k5w_walk_order, dim3(c.n_frames), dim3(kWalkThreads), 0, s, c);
}

}  // namespace ilcc
