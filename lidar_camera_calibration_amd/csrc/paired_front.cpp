// paired_front.cpp -- the front end the paired chains share (paired_front.h).  The layers below do the work: the topic iterator
// (bag_reader.cpp), the pairing (paired_host.cpp), the cut (paired_cut.cpp), K0b (k0b_unpack_batch.hip), K11c
// (k11_camera_image.hip).  Failures are reported through ilcc_last_error(NULL).
#include "paired_front.h"

#include <algorithm>
#include <string>

namespace ilcc {

int32_t PairedRecording::open(const char* entry, const char* image_bag, const char* image_topic, const char* lidar_bag, const char* lidar_topic,
                              const ilcc_camera_model* camera, const double* T, uint64_t first, uint64_t stride, uint64_t max_scans, uint64_t max_dt_ns) {
  if (camera->width <= 0 || camera->height <= 0) return fail(ILCC_BAD_ARGUMENT, "the camera's width and height must be positive");
  int32_t st = ilcc_bag_topic_open(lidar_bag, lidar_topic, nullptr, &clouds.it);
  if (st != ILCC_OK) return st;
  if ((st = open_image_topic(image_bag, image_topic, entry, "", &images.it)) != ILCC_OK) return st;
  const int32_t w = camera->width, h = camera->height;
  proj = ilcc_projection{{T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]}, {T[3], T[7], T[11]}, camera->fx, camera->cx, camera->fy, camera->cy, w, h};
  bgr_image_bytes = align256(3ull * (uint64_t)w * (uint64_t)h);

  // every image's header, once
  const uint64_t n_images = ilcc_bag_topic_count(images.it);
  uint64_t bytes = 0;
  image_of_topic.resize(n_images);
  std::vector<uint64_t> image_ns(n_images);
  for (uint64_t j = 0; j < n_images; ++j) {
    if ((st = read_message(images.it, j, &msg, &bytes)) != ILCC_OK) return st;
    ilcc_image_layout& I = image_of_topic[j];
    if ((st = ilcc_image_parse_any(msg.data(), bytes, &I)) != ILCC_OK) return st;
    if ((int64_t)I.width != w || (int64_t)I.height != h)
      return fail(ILCC_BAD_ARGUMENT, "image message " + std::to_string(j) + " is " + std::to_string(I.width) + " x " + std::to_string(I.height) +
                                         ", the camera " + std::to_string(w) + " x " + std::to_string(h));
    if (I.step > (uint32_t)INT32_MAX) return fail(ILCC_BAD_ARGUMENT, "image step too large");
    image_ns[j] = stamp_ns(I.stamp_sec, I.stamp_nsec);
  }

  // the selected clouds' headers, once; then the pairing
  if ((st = select_messages(clouds.it, first, stride, max_scans, "max_scans", &selected)) != ILCC_OK) return st;
  const uint32_t n_sel = (uint32_t)selected.size();
  cloud_of.resize(n_sel);
  std::vector<uint64_t> cloud_ns(n_sel);
  for (uint32_t s = 0; s < n_sel; ++s) {
    if ((st = read_message(clouds.it, selected[s], &msg, &bytes)) != ILCC_OK) return st;
    if ((st = ilcc_pointcloud2_parse(msg.data(), bytes, &cloud_of[s])) != ILCC_OK) return st;
    cloud_ns[s] = stamp_ns(cloud_of[s].stamp_sec, cloud_of[s].stamp_nsec);
  }
  pair.assign(n_sel, -1);
  dt.assign(n_sel, 0);
  st = ilcc_pair_by_stamp(cloud_ns.data(), n_sel, image_ns.data(), n_images, max_dt_ns, pair.data(), dt.data());
  if (st != ILCC_OK) return fail(st, "pairing failed");
  nearest.assign(n_sel, -1);
  std::vector<int64_t> unused(n_sel, 0);
  (void)ilcc_pair_by_stamp(cloud_ns.data(), n_sel, image_ns.data(), n_images, UINT64_MAX, nearest.data(), unused.data());
  return ILCC_OK;
}

uint32_t PairedRecording::n_paired() const {
  return (uint32_t)std::count_if(pair.begin(), pair.end(), [](int64_t j) { return j >= 0; });
}

int32_t PairedRecording::cut(PairedBudgets budgets, std::vector<PairedBatch>* batches, PairedLargest* largest) const {
  if (!budgets.staging) budgets.staging = kDefaultPairedStagingBytes;
  if (!budgets.image) budgets.image = kDefaultPairedImageBytes;
  std::vector<PairedScan> scans(selected.size());
  for (size_t s = 0; s < scans.size(); ++s) scans[s] = PairedScan{cloud_of[s].data_bytes, (uint64_t)cloud_of[s].height * cloud_of[s].width, pair[s]};
  std::vector<uint64_t> raw(image_of_topic.size());
  for (size_t j = 0; j < raw.size(); ++j) raw[j] = align256((uint64_t)image_of_topic[j].step * image_of_topic[j].height);
  std::string why;
  const int32_t st = paired_cut(scans.data(), (uint32_t)scans.size(), raw.data(), bgr_image_bytes, budgets, batches, largest, &why);
  return st == ILCC_OK ? ILCC_OK : fail(st, why);
}

int32_t PairedBuffers::allocate(const PairedLargest& largest) {
  hipError_t e;
  const uint64_t blob = std::max<uint64_t>(largest.blob_bytes, 16), raw = std::max<uint64_t>(largest.raw_bytes, 16);
  if ((e = hipHostMalloc((void**)&h_blob.p, blob, hipHostMallocDefault)) != hipSuccess || (e = hipHostMalloc((void**)&h_raw.p, raw, hipHostMallocDefault)) != hipSuccess ||
      (e = hipMalloc(&d_blob.p, blob)) != hipSuccess || (e = hipMalloc(&d_xyzi.p, 16 * std::max<uint64_t>(largest.points, 1))) != hipSuccess ||
      (e = hipMalloc(&d_raw.p, raw)) != hipSuccess || (e = hipMalloc(&d_bgr.p, std::max<uint64_t>(largest.bgr_bytes, 16))) != hipSuccess)
    return hip_fail(e);
  return (unpack = ilcc_unpack_plan_create(std::max<uint32_t>(largest.members, 1))) ? ILCC_OK : ILCC_HIP_ERROR;
}

int32_t PairedRecording::stage(PairedBuffers* B, const PairedBatch& b) {
  B->batch = &b;
  B->src.clear();
  B->layouts.clear();
  uint64_t at = 0, bytes = 0;
  for (uint32_t g : b.members) {
    const ilcc_pointcloud2_layout& L = cloud_of[g];
    const int32_t st = read_message(clouds.it, selected[g], &msg, &bytes);
    if (st != ILCC_OK) return st;
    if (L.data_offset + L.data_bytes > bytes) return fail(ILCC_IO_ERROR, "a cloud message changed between two reads of the bag");
    at = align16(at);
    if (L.data_bytes) std::memcpy(B->h_blob.p + at, msg.data() + L.data_offset, L.data_bytes);
    B->src.push_back(at);
    B->layouts.push_back(L);
    at += L.data_bytes;
  }
  for (const ImageSlot& slot : b.images) {
    const ilcc_image_layout& I = image_of_topic[slot.image];
    const int32_t st = read_message(images.it, slot.image, &msg, &bytes);
    if (st != ILCC_OK) return st;
    if (I.data_offset + (uint64_t)I.step * I.height > bytes) return fail(ILCC_IO_ERROR, "an image message changed between two reads of the bag");
    std::memcpy(B->h_raw.p + slot.raw_at, msg.data() + I.data_offset, (uint64_t)I.step * I.height);
  }
  return ILCC_OK;
}

int32_t PairedRecording::upload(PairedBuffers* B, const ilcc_camera_model* lens, hipStream_t s, PairedImages* out) const {
  const PairedBatch& b = *B->batch;
  const uint32_t m = (uint32_t)b.members.size();
  hipError_t e;
  if (b.blob_bytes && (e = hipMemcpyAsync(B->d_blob.p, B->h_blob.p, b.blob_bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e);
  B->offsets.assign(m + 1, 0);
  int32_t st = ilcc_pointcloud2_unpack_batch_device(B->d_blob.p, b.blob_bytes, B->layouts.data(), B->src.data(), m, B->d_xyzi.p, b.points, B->offsets.data(),
                                                    B->unpack, s);
  if (st != ILCC_OK) return st;
  out->image_ptrs.clear();
  out->steps.clear();
  out->image_of_scan.assign(m, -1);
  for (const ImageSlot& slot : b.images) {
    const ilcc_image_layout& I = image_of_topic[slot.image];
    uint8_t* raw = static_cast<uint8_t*>(B->d_raw.p) + slot.raw_at;
    uint8_t* bgr = static_cast<uint8_t*>(B->d_bgr.p) + slot.bgr_at;
    if ((e = hipMemcpyAsync(raw, B->h_raw.p + slot.raw_at, (uint64_t)I.step * I.height, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_fail(e);
    st = ilcc_image_to_bgr8_device(raw, (int32_t)I.width, (int32_t)I.height, (int32_t)I.step, (int32_t)I.encoding, lens, bgr, 3 * (int32_t)I.width, s);
    if (st != ILCC_OK) return st;
    for (uint32_t k = 0; k < m; ++k)
      if (pair[b.members[k]] == (int64_t)slot.image) out->image_of_scan[k] = (int32_t)out->image_ptrs.size();
    out->image_ptrs.push_back(bgr);
    out->steps.push_back(3u * I.width);
  }
  return ILCC_OK;
}

}  // namespace ilcc
