// jpeg_write_sequence_api.cpp -- ilcc_bag_save_jpeg_all (include/ilcc_jpeg_write_sequence.h): every selected image of a bag topic
// through K11, K14b and K17 into one .jpg each.  The layers below do the work: the topic iterator (bag_reader.cpp), the message and
// JPEG header parsers (camera_image_host.cpp, jpeg_host.cpp, jpeg_entropy.cpp), for a CompressedImage topic the host decode pool and
// K13b (jpeg_decode_pool.cpp, k13b_jpeg_batch.hip), K11 (k11_camera_image.hip), K14b (k14b_jpeg_write_batch.hip), K17
// (k17_jpeg_huffman_enc.hip), the cut (image_sequence_host.cpp), and "rows and scans of a batch -> each image's file" with the
// headers and the host encoder (jpeg_finish.h, jpeg_entropy_enc.cpp).  This file owns the batching: one set of buffers sized by
// the largest batch, one stream, and per batch one H2D copy of the staged messages, the launches, the rows back, and ONE copy of
// the scans that were produced.  The guards, the selection and "message i in a vector" are host_util.h's.  Failures below are
// reported through ilcc_last_error(NULL).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_util.h"
#include "ilcc_image_sequence.h"
#include "ilcc_jpeg_sequence.h"
#include "ilcc_jpeg_write.h"
#include "ilcc_jpeg_write_sequence.h"
#include "ilcc_sequence.h"
#include "jpeg_entropy.h"
#include "jpeg_finish.h"

using namespace ilcc;

namespace {

constexpr uint64_t kQuantBytes = 3 * 64 * sizeof(uint16_t);   // a decoded image's table rows
std::string message_name(uint64_t message) { return "message " + std::to_string(message); }

// what one written image takes on the device, every part a multiple of 256
struct Sizes {
  uint64_t mono, coef, out, rows, scratch, device;
};

bool sizes_of(const ilcc_jpeg_info& I, uint64_t out_per_image, Sizes* S) {
  S->mono = align256((uint64_t)I.width * (uint64_t)I.height);
  S->coef = align256(I.coef_count * sizeof(int16_t));
  S->out = align256(align16(out_per_image));
  S->rows = 256;
  S->scratch = ilcc_jpeg_huffman_encode_scratch_bytes(&I, 1, align16(out_per_image));
  S->device = S->mono + S->coef + S->out + S->rows + S->scratch;
  return S->scratch != 0;
}

int32_t write_file(const std::string& path, const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t nb, const uint8_t* c, uint64_t nc) {
  FILE* f = std::fopen(path.c_str(), "wb");
  bool ok = f != nullptr;
  if (f) {
    ok = std::fwrite(a, 1, na, f) == na && (nb == 0 || std::fwrite(b, 1, nb, f) == nb) && (nc == 0 || std::fwrite(c, 1, nc, f) == nc);
    ok = (std::fclose(f) == 0) && ok;
  }
  return ok ? ILCC_OK : fail(ILCC_IO_ERROR, "can not write " + path);
}

int32_t save_all(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera, const char* prefix, int32_t quality,
                 const ilcc_jpeg_write_sequence_params& sp, ilcc_jpeg_write_sequence_result* out, ilcc_jpeg_write_record* records_out, uint32_t cap) {
  Iterator iter;
  bool compressed = false;
  int32_t st = ilcc_bag_topic_open(bag_path, topic, kImageMd5, &iter.it);
  if (st == ILCC_BAD_ARGUMENT) {   // no sensor_msgs/Image there (or an argument both refuse alike): the topic's CompressedImages
    st = ilcc_bag_topic_open(bag_path, topic, kCompressedImageMd5, &iter.it);
    compressed = true;
  }
  if (st != ILCC_OK) return st;
  std::vector<uint64_t> selected;
  if ((st = select_messages(iter.it, sp.first, sp.stride, sp.max_images, "max_images", &selected)) != ILCC_OK) return st;
  const uint32_t n_sel = (uint32_t)selected.size();
  out->n_images = (int32_t)n_sel;
  if (cap < n_sel && (records_out || cap)) return fail(ILCC_CAPACITY, "records holds fewer rows than images were selected");

  // message k of the selection and what its headers say: L for an Image; C and J for a CompressedImage
  std::vector<uint8_t> msg;
  struct Parsed {
    ilcc_image_layout L;
    ilcc_compressed_image_layout C;
    ilcc_jpeg_info J;
  };
  auto read = [&](uint32_t k, Parsed* P) -> int32_t {
    uint64_t bytes = 0;
    int32_t s = read_message(iter.it, selected[k], &msg, &bytes);
    if (s != ILCC_OK) return s;
    if (!compressed) s = ilcc_image_parse_any(msg.data(), bytes, &P->L);
    else if ((s = ilcc_compressed_image_parse(msg.data(), bytes, &P->C)) == ILCC_OK) s = ilcc_jpeg_parse(msg.data() + P->C.data_offset, P->C.data_bytes, &P->J);
    return s == ILCC_OK ? ILCC_OK : fail(s, message_name(selected[k]) + ": " + ilcc_last_error(nullptr));
  };

  // the first selected image decides size and encoding (a JPEG: size, component count and sampling)
  Parsed first;
  if ((st = read(0, &first)) != ILCC_OK) return st;
  if (!compressed && (first.L.width > 65535u || first.L.height > 65535u || first.L.step > (uint32_t)INT32_MAX))
    return fail(ILCC_BAD_ARGUMENT, message_name(selected[0]) + ": image larger than 65535 pixels a side");
  const int32_t w = compressed ? first.J.width : (int32_t)first.L.width, h = compressed ? first.J.height : (int32_t)first.L.height;
  if (camera && (camera->width != w || camera->height != h))
    return fail(ILCC_BAD_ARGUMENT, message_name(selected[0]) + ": the camera's width / height differ from the image's");
  ilcc_jpeg_info I;   // of every file written: one component, no restart markers, as ilcc_bag_save_jpeg writes
  if ((st = ilcc_jpeg_write_info(w, h, 1, 1, 1, quality, 0, &I)) != ILCC_OK) return st;
  const uint64_t out_per_image = align16(sp.out_bytes_per_image ? sp.out_bytes_per_image : (uint64_t)w * (uint64_t)h);
  Sizes S;
  if (!sizes_of(I, out_per_image, &S)) return fail(ILCC_BAD_ARGUMENT, message_name(selected[0]) + ": image too large for K17");
  // a CompressedImage is decoded as in ilcc_jpeg_sequence.h: its coefficients and table rows are staged, K13b makes the pixels
  const int32_t src_bpp = compressed && first.J.n_components == 3 ? 3 : 1;
  uint64_t src_coef = 0, src_planes = 0, src_pixels = 0, src_staged = 0;
  if (compressed) {
    if (!jpeg_laid_out(first.J)) return fail(ILCC_BAD_ARGUMENT, message_name(selected[0]) + ": the JPEG's layout is not ilcc_jpeg_layout's");
    src_coef = align256(first.J.coef_count * sizeof(int16_t));
    src_staged = src_coef + align256(kQuantBytes);
    src_planes = ilcc_jpeg_scratch_bytes(&first.J);
    src_pixels = align256((uint64_t)src_bpp * (uint64_t)w * (uint64_t)h);
  }

  // the batches, cut before anything is allocated
  std::vector<uint64_t> raw(n_sel, src_staged);
  if (!compressed)
    for (uint32_t k = 0; k < n_sel; ++k) {
      st = ilcc_bag_topic_read(iter.it, selected[k], nullptr, 0, &raw[k]);
      if (st != ILCC_OK && st != ILCC_CAPACITY) return st;
    }
  const uint64_t per_image = S.device + src_planes + src_pixels;   // beside what it stages, which the blob holds on both sides
  std::vector<uint32_t> batch_first(n_sel + 1);
  uint32_t n_batches = 0;
  st = ilcc_image_sequence_cut(raw.data(), n_sel, per_image, sp.staging_bytes, sp.device_bytes, batch_first.data(), &n_batches);
  if (st == ILCC_CAPACITY)
    return fail(st, "one image (" + std::to_string(per_image) + " device bytes, messages up to " + std::to_string(*std::max_element(raw.begin(), raw.end())) +
                        " staged bytes) is above staging_bytes or device_bytes");
  if (st != ILCC_OK) return fail(st, "the selection could not be cut into batches");
  uint64_t blob_cap = 256;
  uint32_t images_cap = 1;
  for (uint32_t b = 0; b < n_batches; ++b) {
    uint64_t bytes = 0;
    for (uint32_t k = batch_first[b]; k < batch_first[b + 1]; ++k) bytes += align256(raw[k]);
    blob_cap = std::max(blob_cap, bytes);
    images_cap = std::max(images_cap, batch_first[b + 1] - batch_first[b]);
  }

  std::vector<ilcc_jpeg_write_record> records(n_sel);
  std::memset(static_cast<void*>(records.data()), 0, sizeof(ilcc_jpeg_write_record) * n_sel);

  // one set of allocations for the whole call: [ blob | planes | pixels | mono8 | coefficients | scans | rows | K17's scratch ]
  if ((st = select_device(device)) != ILCC_OK) return st;
  hipError_t e;
  Stream stream;
  if ((e = hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking)) != hipSuccess) return hip_fail(e);
  const uint64_t out_cap_max = out_per_image * images_cap, coef_pitch = S.coef / sizeof(int16_t);
  const uint64_t k17_scratch = ilcc_jpeg_huffman_encode_scratch_bytes(&I, images_cap, out_cap_max);
  const uint64_t planes_at = align256(blob_cap), pixels_at = planes_at + src_planes * images_cap, mono_at = pixels_at + src_pixels * images_cap;
  const uint64_t coef_at = mono_at + S.mono * images_cap, out_at = coef_at + S.coef * images_cap, rows_at = out_at + align256(out_cap_max);
  const uint64_t scratch_at = rows_at + align256(sizeof(ilcc_jpeg_encode_row) * images_cap);
  DeviceBuffer d_all;
  Pinned h_blob, h_back;   // h_back: [ rows | scans ]
  const uint64_t back_rows = align256(sizeof(ilcc_jpeg_encode_row) * images_cap);
  if ((e = hipMalloc(&d_all.p, scratch_at + k17_scratch)) != hipSuccess || (e = hipHostMalloc((void**)&h_blob.p, blob_cap, hipHostMallocDefault)) != hipSuccess ||
      (e = hipHostMalloc((void**)&h_back.p, back_rows + out_cap_max, hipHostMallocDefault)) != hipSuccess)
    return hip_fail(e);
  uint8_t* base = (uint8_t*)d_all.p;

  JpegFinisher files;   // K17's rows and scans of a batch -> each image's file
  files.info = &I;
  files.stream = stream.s;
  files.d_coef = base + coef_at;
  files.coef_pitch = S.coef;
  files.d_scans = base + out_at;
  files.d_rows = reinterpret_cast<const ilcc_jpeg_encode_row*>(base + rows_at);
  files.out_per_image = out_per_image;
  files.h_back = h_back.p;
  files.back_rows = back_rows;
  if ((st = files.init()) != ILCC_OK) return st;
  std::vector<uint8_t> encoded;   // of an image the host encodes

  std::vector<Parsed> parsed(images_cap);
  std::vector<uint64_t> at(images_cap);
  std::vector<const uint8_t*> jpg(images_cap);
  std::vector<uint64_t> jpg_bytes(images_cap), coef_room(images_cap, compressed ? first.J.coef_count : 0);
  std::vector<int16_t*> coef_to(images_cap);
  std::vector<int32_t> decode_status(images_cap);
  std::vector<std::vector<uint8_t>> kept(compressed ? images_cap : 0);   // the messages stay while the pool reads them

  for (uint32_t bi = 0; bi < n_batches; ++bi) {
    const uint32_t b0 = batch_first[bi], n = batch_first[bi + 1] - b0;
    // stage: an Image's data[] at 256-byte aligned offsets of the blob; a CompressedImage's coefficients, then the batch's table rows
    uint64_t bytes = 0;
    for (uint32_t m = 0; m < n; ++m) {
      const uint32_t k = b0 + m;
      Parsed& P = parsed[m];
      if ((st = read(k, &P)) != ILCC_OK) return st;
      const uint32_t pw = compressed ? (uint32_t)P.J.width : P.L.width, ph = compressed ? (uint32_t)P.J.height : P.L.height;
      if ((int32_t)pw != w || (int32_t)ph != h)
        return fail(ILCC_BAD_ARGUMENT, message_name(selected[k]) + ": image " + std::to_string(pw) + " x " + std::to_string(ph) + " differs from the first selected image's " +
                                           std::to_string(w) + " x " + std::to_string(h));
      ilcc_jpeg_write_record& r = records[k];
      r.message = (uint32_t)selected[k];
      (void)ilcc_bag_topic_time(iter.it, selected[k], &r.time_sec, &r.time_nsec);
      if (!compressed) {
        if (P.L.encoding != first.L.encoding) return fail(ILCC_BAD_ARGUMENT, message_name(selected[k]) + ": its encoding differs from the first selected image's");
        if (P.L.step > (uint32_t)INT32_MAX || bytes + P.L.data_bytes > blob_cap)
          return fail(ILCC_BAD_ARGUMENT, message_name(selected[k]) + ": image data[] larger than its message");
        at[m] = bytes;
        std::memcpy(h_blob.p + bytes, msg.data() + P.L.data_offset, P.L.data_bytes);
        bytes = align256(bytes + P.L.data_bytes);
        r.stamp_sec = P.L.stamp_sec;
        r.stamp_nsec = P.L.stamp_nsec;
      } else {
        if (P.J.n_components != first.J.n_components || P.J.comp[0].h != first.J.comp[0].h || P.J.comp[0].v != first.J.comp[0].v ||
            P.J.coef_count != first.J.coef_count)
          return fail(ILCC_BAD_ARGUMENT, message_name(selected[k]) + ": its component count or chroma sampling differs from the first selected image's");
        kept[m].swap(msg);
        jpg[m] = kept[m].data() + P.C.data_offset;
        jpg_bytes[m] = P.C.data_bytes;
        coef_to[m] = reinterpret_cast<int16_t*>(h_blob.p + src_coef * m);
        uint16_t* quant = reinterpret_cast<uint16_t*>(h_blob.p + src_coef * n) + (size_t)m * 3 * 64;
        for (int c = 0; c < 3; ++c)   // a 1-component image: row 0 three times
          std::memcpy(quant + c * 64, P.J.quant[P.J.comp[c < P.J.n_components ? c : 0].quant_index], 64 * sizeof(uint16_t));
        r.stamp_sec = P.C.stamp_sec;
        r.stamp_nsec = P.C.stamp_nsec;
      }
    }
    if (compressed) {
      std::vector<ilcc_jpeg_info> infos(n);
      for (uint32_t m = 0; m < n; ++m) infos[m] = parsed[m].J;
      st = ilcc_jpeg_entropy_decode_many(jpg.data(), jpg_bytes.data(), infos.data(), coef_to.data(), coef_room.data(), n, 0, decode_status.data());
      if (st != ILCC_OK) {
        uint32_t m = 0;
        while (m + 1 < n && decode_status[m] == ILCC_OK) ++m;
        return fail(st, message_name(selected[b0 + m]) + ": " + ilcc_last_error(nullptr));
      }
      bytes = src_coef * n + kQuantBytes * n;
    }
    if ((e = hipMemcpyAsync(base, h_blob.p, std::min(bytes, blob_cap), hipMemcpyHostToDevice, stream.s)) != hipSuccess) return hip_fail(e);
    if (compressed) {
      st = ilcc_jpeg_idct_batch_device(&first.J, reinterpret_cast<const uint16_t*>(base + src_coef * n), reinterpret_cast<const int16_t*>(base),
                                       src_coef / sizeof(int16_t), n, base + pixels_at, src_pixels, src_bpp * w, base + planes_at, src_planes * images_cap, stream.s);
      if (st != ILCC_OK) return st;
    }
    // K11 per image into the packed mono8 array, K14b, and on route 0 K17: all on the call's stream
    for (uint32_t m = 0; m < n; ++m) {
      if (compressed)
        st = ilcc_image_to_mono8_device(base + pixels_at + src_pixels * m, w, h, src_bpp * w, src_bpp == 1 ? ILCC_ENCODING_MONO8 : ILCC_ENCODING_BGR8, camera,
                                        base + mono_at + S.mono * m, w, stream.s);
      else
        st = ilcc_image_to_mono8_device(base + at[m], w, h, (int32_t)parsed[m].L.step, (int32_t)parsed[m].L.encoding, camera, base + mono_at + S.mono * m, w,
                                        stream.s);
      if (st != ILCC_OK) return fail(st, message_name(selected[b0 + m]) + ": " + ilcc_last_error(nullptr));
    }
    ilcc_jpeg_fdct_batch_job fj{};
    fj.layout = &I;
    fj.d_src = base + mono_at;
    fj.image_pitch = S.mono;
    fj.src_stride = w;
    fj.encoding = ILCC_ENCODING_MONO8;
    fj.d_coef = reinterpret_cast<int16_t*>(base + coef_at);
    fj.coef_pitch = coef_pitch;
    fj.n_images = n;
    fj.hip_stream = stream.s;
    if ((st = ilcc_jpeg_fdct_batch_device(&fj)) != ILCC_OK) return st;
    if (sp.route == 0) {
      ilcc_jpeg_huffman_encode_job hj{};
      hj.layout = &I;
      hj.d_coef = fj.d_coef;
      hj.coef_pitch = coef_pitch;
      hj.d_out = base + out_at;
      hj.out_cap = out_per_image * n;
      hj.d_rows = reinterpret_cast<ilcc_jpeg_encode_row*>(base + rows_at);
      hj.d_scratch = base + scratch_at;
      hj.scratch_bytes = k17_scratch;
      hj.n_images = n;
      hj.hip_stream = stream.s;
      if ((st = ilcc_jpeg_huffman_encode_batch_device(&hj)) != ILCC_OK) return st;
      // the rows, then one copy of the scans that were produced
      if ((st = files.rows_back(n)) != ILCC_OK) return st;
      if ((e = hipStreamSynchronize(stream.s)) != hipSuccess) return hip_fail(e);
      bool queued = false;
      if ((st = files.scans_back(n, &queued)) != ILCC_OK) return st;
      if (queued && (e = hipStreamSynchronize(stream.s)) != hipSuccess) return hip_fail(e);
    }
    for (uint32_t m = 0; m < n; ++m) {   // the file's spans go to fwrite as they are: nothing assembles them
      JpegFile f;
      if ((st = files.file(m, sp.route, message_name(selected[b0 + m]), &encoded, &f)) != ILCC_OK) return st;
      ilcc_jpeg_write_record& r = records[b0 + m];
      r.route = f.route;
      r.file_bytes = f.bytes();
      char number[16];
      std::snprintf(number, sizeof(number), "%06u", (unsigned)selected[b0 + m]);
      st = write_file(std::string(prefix) + number + ".jpg", f.part[0], f.part_bytes[0], f.part[1], f.part_bytes[1], f.part[2], f.part_bytes[2]);
      if (st != ILCC_OK) return st;
    }
    out->d2h_bytes = files.d2h_bytes;
    out->n_host_encoded = files.n_host_encoded;
    ++out->n_batches;
  }
  for (uint32_t k = 0; k < n_sel; ++k) {
    out->file_bytes += records[k].file_bytes;
    if (records_out) records_out[k] = records[k];
  }
  return ILCC_OK;
}

}  // namespace

extern "C" {

void ilcc_default_jpeg_write_sequence_params(ilcc_jpeg_write_sequence_params* sp) {
  if (sp) std::memset(sp, 0, sizeof(*sp));
}

uint64_t ilcc_jpeg_write_sequence_bytes(int32_t width, int32_t height, uint64_t out_bytes_per_image) {
  ilcc_jpeg_info I;
  Sizes S;
  if (ilcc_jpeg_write_info(width, height, 1, 1, 1, 95, 0, &I) != ILCC_OK) return 0;
  return sizes_of(I, align16(out_bytes_per_image ? out_bytes_per_image : (uint64_t)width * (uint64_t)height), &S) ? S.device : 0;
}

int32_t ilcc_bag_save_jpeg_all(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera, const char* path_prefix,
                               int32_t quality, const ilcc_jpeg_write_sequence_params* sp, ilcc_jpeg_write_sequence_result* out,
                               ilcc_jpeg_write_record* records, uint32_t cap) {
  if (!out) return fail(ILCC_BAD_ARGUMENT, "null argument");
  std::memset(out, 0, sizeof(*out));
  int32_t st;
  if (!bag_path || !topic || !path_prefix || !sp || (records == nullptr && cap != 0)) {
    st = fail(ILCC_BAD_ARGUMENT, "null argument");
  } else if (sp->route > 1) {
    st = fail(ILCC_BAD_ARGUMENT, "route must be 0, K17, or 1, the host encoder");
  } else {
    try {   // no exception crosses the C-ABI
      st = save_all(device, bag_path, topic, camera, path_prefix, quality, *sp, out, records, cap);
    } catch (const std::bad_alloc&) {
      st = fail(ILCC_IO_ERROR, "out of memory");
    } catch (...) {
      st = fail(ILCC_IO_ERROR, "jpeg write sequence: unknown failure");
    }
  }
  out->status = st;
  return st;
}

}  // extern "C"
