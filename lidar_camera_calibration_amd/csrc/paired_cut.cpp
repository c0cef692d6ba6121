// paired_cut.cpp -- the batch cut of the paired chains (paired_cut.h).  Plain C++ without HIP.
#include "paired_cut.h"

#include <algorithm>

#include "ilcc_hip.h"

namespace ilcc {

int32_t paired_cut(const PairedScan* scans, uint32_t n_scans, const uint64_t* image_raw_bytes, uint64_t bgr_image_bytes, const PairedBudgets& budgets,
                   std::vector<PairedBatch>* batches, PairedLargest* largest, std::string* why) {
  const auto refuse = [&](int32_t code, const std::string& text) {
    *why = text;
    return code;
  };
  const PairedBudgets& B = budgets;
  batches->clear();
  *largest = PairedLargest{};
  if (B.device && B.per_member > B.device) return refuse(ILCC_CAPACITY, "one paired scan (" + std::to_string(B.per_member) + " device bytes) is above device_bytes");
  std::vector<uint32_t> needed;   // the distinct images of the batch being filled
  for (uint32_t s = 0; s < n_scans;) {
    PairedBatch b;
    b.first_scan = s;
    needed.clear();
    uint64_t image_cost = 0, counted = 0;   // counted: the data[] of every scan of the batch, staged or not
    while (s < n_scans) {
      const PairedScan& L = scans[s];
      const bool staged = B.stage_unpaired || L.pair >= 0;
      const uint64_t counted_at = (counted + 15u) & ~(uint64_t)15u, members = b.members.size();
      if (L.data_bytes > B.staging) return refuse(ILCC_CAPACITY, "a scan's data[] is larger than staging_bytes");
      const bool new_image = L.pair >= 0 && std::find(needed.begin(), needed.end(), (uint32_t)L.pair) == needed.end();
      const uint64_t extra = new_image ? image_raw_bytes[L.pair] + bgr_image_bytes : 0;
      if (extra > B.image) return refuse(ILCC_CAPACITY, "an image (raw + B,G,R) is larger than image_bytes");
      if (staged && b.points + L.points > 0xFFFFFFFEull) {
        if (members == 0) return refuse(ILCC_BAD_ARGUMENT, "cloud of more than 2^32 - 2 points");
        break;
      }
      const bool device_full = staged && ((B.device && (members + 1) * B.per_member > B.device) || (B.member_cap && members >= B.member_cap));
      if (b.scans > 0 && (counted_at + L.data_bytes > B.staging || image_cost + extra > B.image || device_full)) break;
      counted = counted_at + L.data_bytes;
      image_cost += extra;
      if (new_image) needed.push_back((uint32_t)L.pair);
      if (staged) {
        b.blob_bytes = ((b.blob_bytes + 15u) & ~(uint64_t)15u) + L.data_bytes;
        b.points += L.points;
        b.members.push_back(s);
      }
      ++b.scans;
      ++s;
    }
    for (uint32_t j : needed) {
      b.images.push_back(ImageSlot{j, b.raw_bytes, b.bgr_bytes});
      b.raw_bytes += image_raw_bytes[j];
      b.bgr_bytes += bgr_image_bytes;
    }
    largest->members = std::max<uint32_t>(largest->members, (uint32_t)b.members.size());
    largest->blob_bytes = std::max(largest->blob_bytes, b.blob_bytes);
    largest->points = std::max(largest->points, b.points);
    largest->raw_bytes = std::max(largest->raw_bytes, b.raw_bytes);
    largest->bgr_bytes = std::max(largest->bgr_bytes, b.bgr_bytes);
    batches->push_back(std::move(b));
  }
  return ILCC_OK;
}

}  // namespace ilcc
