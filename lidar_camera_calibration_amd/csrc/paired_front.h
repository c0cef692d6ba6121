// The front end the paired chains share (paired_api.cpp, overlay_sequence_api.cpp): a recording's selected scans, each paired with
// the image whose header stamp is nearest; the batches (paired_cut.h); and per batch the staging of its messages, their upload,
// K0b and K11c.  What a chain does with a batch's points and B,G,R images is its own.  Internal, not installed.
#pragma once

#include <cstring>
#include <vector>

#include "host_util.h"
#include "ilcc_paired.h"
#include "paired_cut.h"

namespace ilcc {

// the common part of one of a chain's two sets of buffers
struct PairedBuffers {
  Pinned h_blob, h_raw;
  DeviceBuffer d_blob, d_xyzi, d_raw, d_bgr;
  ilcc_unpack_plan* unpack = nullptr;
  std::vector<uint64_t> src, offsets;             // per member: where its data[] lies in the blob; where its points lie in d_xyzi
  std::vector<ilcc_pointcloud2_layout> layouts;   // per member
  const PairedBatch* batch = nullptr;
  ~PairedBuffers() { ilcc_unpack_plan_destroy(unpack); }
  int32_t allocate(const PairedLargest& largest);
};

// what upload() made of a batch's images, for the chain's own kernel; valid while the buffers carry the batch
struct PairedImages {
  std::vector<const void*> image_ptrs;   // B,G,R on the device, per image slot
  std::vector<uint32_t> steps;
  std::vector<int32_t> image_of_scan;    // per member: its slot, -1 for an unpaired one
};

struct PairedRecording {
  Iterator clouds, images;
  std::vector<uint64_t> selected;                  // cloud message indices
  std::vector<ilcc_pointcloud2_layout> cloud_of;   // per selected scan
  std::vector<ilcc_image_layout> image_of_topic;   // per image message
  std::vector<int64_t> pair, dt, nearest;          // per selected scan; nearest: the pairing without a limit, for an unpaired scan's record
  ilcc_projection proj{};
  uint64_t bgr_image_bytes = 0;
  std::vector<uint8_t> msg;

  // everything from the two opens to the pairing: every image's header and every selected cloud's are read once.  `entry` names the
  // caller in the CompressedImage refusal.
  int32_t open(const char* entry, const char* image_bag, const char* image_topic, const char* lidar_bag, const char* lidar_topic,
               const ilcc_camera_model* camera, const double* T, uint64_t first, uint64_t stride, uint64_t max_scans, uint64_t max_dt_ns);
  uint32_t n_paired() const;
  // the batches; budgets.staging and .image are the chain's parameters, 0 for the defaults the two chains share
  int32_t cut(PairedBudgets budgets, std::vector<PairedBatch>* batches, PairedLargest* largest) const;
  // host only: the members' data[] and the images of the batch into the page-locked buffers
  int32_t stage(PairedBuffers* B, const PairedBatch& b);
  // queued on s: the blob's copy, K0b, and per image slot the raw copy and K11c (lens: nullptr samples the raw image)
  int32_t upload(PairedBuffers* B, const ilcc_camera_model* lens, hipStream_t s, PairedImages* out) const;

  // the fields ilcc_pair_record and ilcc_overlay_record have in common, of selected scan g; the others zero
  template <class Record>
  void fill(uint32_t g, Record* r) const {
    std::memset(r, 0, sizeof(*r));
    r->message = (uint32_t)selected[g];
    r->stamp_sec = cloud_of[g].stamp_sec;
    r->stamp_nsec = cloud_of[g].stamp_nsec;
    r->image_message = (int32_t)pair[g];
    if (nearest[g] >= 0) {
      r->image_stamp_sec = image_of_topic[nearest[g]].stamp_sec;
      r->image_stamp_nsec = image_of_topic[nearest[g]].stamp_nsec;
    }
    r->dt_ns = dt[g];
    r->n_points = (uint64_t)cloud_of[g].height * cloud_of[g].width;
  }
};

constexpr uint64_t kDefaultPairedStagingBytes = 256ull << 20, kDefaultPairedImageBytes = 512ull << 20;

}  // namespace ilcc
