// The K18 route of structure recovery in the image chains (image_sequence_api.cpp, jpeg_sequence_api.cpp;
// ilcc_image_sequence_params.reserved0 == 1): a batch's corner lists through ilcc_chessboards_from_corners_batch on the call's
// stream, right after the batch's K10b, and the boards into the batch's records as the host route writes them.  One plan per call,
// sized like the chain's buffers; it is made again only when a batch's corner capacity has grown.  Internal, not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <vector>

#include "host_util.h"
#include "ilcc_image_sequence.h"
#include "ilcc_image_structure.h"

namespace ilcc {

struct StructureRoute {
  ilcc_structure_plan* plan = nullptr;
  uint32_t plan_images = 0;
  int32_t plan_corners = 0;
  std::vector<int32_t> status, rows, cols, idx;
  double ms = 0;   // wall time spent here, all batches
  ~StructureRoute() { ilcc_structure_plan_destroy(plan); }

  // records: of the batch's first image
  int32_t recover(const ilcc_image_corner* corners, int32_t capacity, const int32_t* n_corners, uint32_t count, uint32_t images_cap, int32_t board_w,
                  int32_t board_h, ilcc_image_record* records, hipStream_t stream) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!plan || plan_images < images_cap || plan_corners < capacity) {
      ilcc_structure_plan_destroy(plan);
      plan_images = images_cap;
      plan_corners = capacity > 1 ? capacity : 1;
      if (!(plan = ilcc_structure_plan_create(plan_images, (uint32_t)plan_corners))) return ILCC_HIP_ERROR;
    }
    const size_t cells = (size_t)board_w * board_h;
    status.assign(count, 0);
    rows.assign(count, 0);
    cols.assign(count, 0);
    idx.assign(count * cells, 0);
    const int32_t st = ilcc_chessboards_from_corners_batch(corners, capacity, n_corners, count, board_w, board_h, status.data(), rows.data(), cols.data(),
                                                           idx.data(), plan, stream);
    if (st != ILCC_OK) return st;
    for (uint32_t m = 0; m < count; ++m) {
      ilcc_image_record& r = records[m];
      const ilcc_image_corner* c = corners + (size_t)m * capacity;
      r.n_corners = n_corners[m];
      r.status = status[m];
      if (r.status != ILCC_OK) continue;
      r.rows = rows[m];
      r.cols = cols[m];
      for (size_t i = 0; i < cells; ++i) {
        r.xy[2 * i] = c[idx[m * cells + i]].u;
        r.xy[2 * i + 1] = c[idx[m * cells + i]].v;
      }
    }
    ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return ILCC_OK;
  }
};

}  // namespace ilcc
