// The batch cut of the paired chains (paired_api.cpp, overlay_sequence_api.cpp): which of a recording's selected scans, each with
// the image it is paired with, form a batch under the chains' budgets.  Numbers in, numbers out: plain C++ without HIP, so that
// it also builds alone, under sanitizers, for tests/test_paired_cpu.py, and tests/paired_ref.py restates it.  Internal, not
// installed, not exported from the library.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace ilcc {

struct PairedScan {
  uint64_t data_bytes, points;
  int64_t pair;   // the image's index on its topic; -1: unpaired
};

struct ImageSlot {           // a distinct image of a batch
  uint32_t image;            // index on the topic
  uint64_t raw_at, bgr_at;   // in the batch's raw / B,G,R regions
};

struct PairedBatch {
  uint32_t first_scan = 0, scans = 0;   // among the selected scans
  std::vector<uint32_t> members;        // the staged ones, as indices among the selected scans: what the device sees
  uint64_t blob_bytes = 0, points = 0, raw_bytes = 0, bgr_bytes = 0;
  std::vector<ImageSlot> images;        // in the order they are first needed
};

struct PairedBudgets {
  uint64_t staging = 0;        // the data[] of a batch's scans, each at a multiple of 16; unpaired scans count whether staged or not
  uint64_t image = 0;          // the distinct images of a batch, raw + B,G,R
  uint64_t device = 0;         // members * per_member; 0: the chain has no device budget
  uint64_t per_member = 0;
  uint32_t member_cap = 0;     // 0: none
  bool stage_unpaired = false; // true: an unpaired scan is a member like any other; false: it costs a record, nothing on the device
};

struct PairedLargest {   // the largest of each over the batches: what one set of buffers must hold
  uint32_t members = 0;
  uint64_t blob_bytes = 0, points = 0, raw_bytes = 0, bgr_bytes = 0;
};

// image_raw_bytes[j]: image j's data[], already a multiple of 256; bgr_image_bytes: an image's B,G,R, likewise.  An image shared by
// two batches is charged to both.  A scan that would take a batch's members past 2^32 - 2 points closes the batch.
// ILCC_CAPACITY: a scan above staging, an image above image, one member above device; ILCC_BAD_ARGUMENT: a batch's first member
// of more than 2^32 - 2 points; *why is the text.
__attribute__((visibility("hidden"))) int32_t paired_cut(const PairedScan* scans, uint32_t n_scans, const uint64_t* image_raw_bytes,
                                                         uint64_t bgr_image_bytes, const PairedBudgets& budgets,
                                                         std::vector<PairedBatch>* batches, PairedLargest* largest, std::string* why);

}  // namespace ilcc
