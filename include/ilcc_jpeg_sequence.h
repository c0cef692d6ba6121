/*
 * ilcc_jpeg_sequence.h -- camera corners from EVERY sensor_msgs/CompressedImage of a recording (in libilcc_hip.so).
 *
 * A camera bag recorded the usual way carries JPEG frames.  ilcc_jpeg.h decodes one of them (K13: four launches, one
 * allocation, one pageable copy and one serial Huffman decode per colour image); ilcc_image_sequence.h fuses the boards of
 * every raw sensor_msgs/Image of a topic.  The entries here join the two: a batch of JPEG frames of one geometry is decoded in
 * two launches (K13b) behind a Huffman decode on several host threads, and goes on through K11, K10b, structure recovery and
 * the fusion exactly as the raw frames of ilcc_bag_corners_all_images do.  Three layers, each usable alone:
 *
 *   single image (ilcc_jpeg.h)                                    here
 *   ------------------------------------------------------------  -----------------------------------------------------
 *   ilcc_jpeg_idct_device on one image (K13)                      ilcc_jpeg_idct_batch_device on n images (K13b,
 *                                                                   csrc/k13b_jpeg_batch.hip; the stage bodies are K13's
 *                                                                   own, csrc/k13_stages.h)
 *   ilcc_jpeg_entropy_decode on the calling thread                ilcc_jpeg_entropy_decode_many on up to 16 threads
 *                                                                   (csrc/jpeg_decode_pool.cpp, plain C++ without HIP)
 *   ilcc_bag_find_chessboard: the first CompressedImage           ilcc_bag_corners_all_compressed_images: every selected
 *                                                                   one, fused (csrc/jpeg_sequence_api.cpp)
 */
#ifndef ILCC_JPEG_SEQUENCE_H_
#define ILCC_JPEG_SEQUENCE_H_

#include "ilcc_image_sequence.h"
#include "ilcc_jpeg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 1. K13b: IDCT, upsampling and colour on a batch of images -------------------------------------------------------------
 * Geometry shared by every image of a batch: width, height, n_components, h / v, blocks_w / blocks_h, coef_offset, coef_count of
 * `layout` (what ilcc_jpeg_layout fills); its quant[] is NOT read.
 * d_quant: [n_images][3][64] uint16, natural order, 16-byte aligned: row c of image m is component c's table (a 1-component
 *          image reads row 0 only).
 * d_coef : image m's coefficients at d_coef + m * coef_pitch (int16 units; coef_pitch >= coef_count, a multiple of 8), laid
 *          out as ilcc_jpeg_entropy_decode leaves them.
 * d_dst  : image m at d_dst + m * dst_pitch (bytes; >= dst_stride * height), mono8 or bgr8, rows dst_stride apart.
 * d_scratch: ilcc_jpeg_batch_scratch_bytes(layout, n_images) bytes, 16-byte aligned (3 components only): image m's three padded
 *          sample planes at d_scratch + m * ilcc_jpeg_scratch_bytes(layout).
 * CONTRACT: every byte of image m equals what ilcc_jpeg_idct_device writes for (layout + image m's tables, image m's coefficients);
 * not a byte outside [row * dst_stride, row * dst_stride + bpp * width) of any image is written.  Asynchronous on hip_stream, no
 * allocation, no host wait; *layout is read before the call returns.  d_scratch belongs to the call until its launches have run.
 * n_images == 0: ILCC_OK, no launch.
 *
 * Launches, whatever n_images is: ONE k13b_idct for all components of all images (the image is blockIdx.z, the (component,
 * block row) pair is flattened into blockIdx.y, blockIdx.x is the 32-block group sized for the widest component), and for 3
 * components ONE k13b_upsample_colour with the image as blockIdx.z.  Two launches per colour batch, one per gray batch.
 *
 * Refusals -- on the host, nothing launched (ILCC_BAD_ARGUMENT): null pointers, a layout ilcc_jpeg_layout would not make,
 * n_images above 65535, a coef_pitch short of coef_count or not a multiple of 8, a misaligned d_coef, d_quant or d_scratch, a
 * dst_stride shorter than a row, a dst_pitch short of dst_stride * height, too little scratch. */
uint64_t ilcc_jpeg_batch_scratch_bytes(const ilcc_jpeg_info* layout, uint32_t n_images);   /* 0 for 1 component / a refused layout */
int32_t  ilcc_jpeg_idct_batch_device(const ilcc_jpeg_info* layout, const uint16_t* d_quant, const int16_t* d_coef, uint64_t coef_pitch,
                                     uint32_t n_images, void* d_dst, uint64_t dst_pitch, int32_t dst_stride,
                                     void* d_scratch, uint64_t scratch_bytes, void* hip_stream);

/* ---- 2. Huffman decoding of a batch on several host threads ------------------------------------------------------------------
 * Decodes jobs 0 .. n-1 (jpg[i], bytes[i], info[i] -> coef[i], cap[i]) on up to `threads` host threads (0: 8; at most 16).
 * status[i] gets each job's status; returns the status of the LOWEST failing job with ITS text in ilcc_last_error, ILCC_OK
 * otherwise.  Results do not depend on `threads`: every job is ilcc_jpeg_entropy_decode on its own arguments, the threads share
 * nothing but the counter they draw jobs from.  Null arrays with n > 0: ILCC_BAD_ARGUMENT.  Host only. */
int32_t ilcc_jpeg_entropy_decode_many(const uint8_t* const* jpg, const uint64_t* bytes, const ilcc_jpeg_info* info,
                                      int16_t* const* coef, const uint64_t* cap, uint32_t n, uint32_t threads, int32_t* status);

/* ---- 3. the chain ---------------------------------------------------------------------------------------------------------- */
typedef struct ilcc_jpeg_sequence_params {
  ilcc_image_sequence_params seq;   /* first / stride / max_images / gate_px / staging_bytes / device_bytes and reserved0 (the route
                                     * of structure recovery: 0 the host thread, 1 K18), as documented there */
  uint32_t decode_threads;          /* 0: 8; above 16 is read as 16 */
  uint32_t reserved0;               /* the route of the Huffman decode: 0 (the default) the host pool below; 1 K16 on the device
                                     * (ilcc_jpeg_huffman.h: the pool's threads then only prepare the scans); anything else is
                                     * ILCC_BAD_ARGUMENT.  The records do not depend on it. */
} ilcc_jpeg_sequence_params;
void    ilcc_default_jpeg_sequence_params(ilcc_jpeg_sequence_params*);

/* staged and device bytes one image of `layout` takes in the chain (host arithmetic; what the chain cuts its batches with).
 * With up(x) = x rounded up to 256 and bpp = 1 or 3:
 *   staged = up(2 * coef_count) + up(2 * 3 * 64)                       coefficients + table rows, what the H2D copy moves
 *   device = staged + ilcc_jpeg_scratch_bytes(layout)                  K13b's planes (0 for 1 component)
 *                   + up(bpp * width * height)                         the decoded pixels, rows packed
 *                   + up(width * height)                               mono8 behind K11
 *                   + ilcc_image_corner_scratch_bytes(width, height)   K10b
 * ILCC_BAD_ARGUMENT: null pointers, a layout ilcc_jpeg_layout would not make. */
int32_t ilcc_jpeg_sequence_bytes(const ilcc_jpeg_info* layout, uint64_t* staged_bytes, uint64_t* device_bytes);

/* Every selected sensor_msgs/CompressedImage of `topic` -> ilcc_compressed_image_parse -> ilcc_jpeg_parse -> entropy decode on the
 * pool -> K13b -> K11 per image into the packed mono8 array (camera NULL: conversion only) -> K10b ->
 * ilcc_chessboard_from_corners -> ilcc_fuse_image_corners.  The first selected image fixes width, height, component count and
 * sampling; quantisation tables, Huffman tables and restart intervals may differ from image to image.  Batches are cut with
 * ilcc_image_sequence_cut before anything is allocated: raw_bytes = `staged` of ilcc_jpeg_sequence_bytes for every image (against
 * seq.staging_bytes), device_bytes_per_image = its `device` (against seq.device_bytes).  Per batch, on the call's one stream:
 * coefficients and tables of all its images decoded straight into one page-locked blob, ONE H2D copy, K13b, K11 per image, K10b
 * (run again with more room when an image holds more corners than expected).  The pool decodes batch k + 1 into the other set of
 * buffers while the device works on batch k and the recovery thread on batch k - 1; two sets, allocated once per call, and only
 * when there is more than one batch.
 * CONTRACT: every record's status, n_corners, rows, cols and xy equal what ilcc_jpeg_decode_device + ilcc_image_to_mono8_device +
 * ilcc_find_chessboard_device give for that message alone, so record 0 with first = 0 equals ilcc_bag_find_chessboard on the same
 * topic.  The records do not depend on decode_threads or on how the batches were cut.
 * Refusals, on the host, with a text that names the message: a topic without any CompressedImage (ILCC_BAD_ARGUMENT; when it
 * carries sensor_msgs/Image the text says that ilcc_bag_corners_all_images takes it); a format that is not JPEG; a JPEG that K13
 * refuses (the decoder's own text behind the message's name); an image whose size, component count or sampling differs from the
 * first selected one's; a camera of another size; a side below 34 px; one image above a budget (ILCC_CAPACITY); per_image_out
 * smaller than the selection (ILCC_CAPACITY with out->n_images = the number needed, nothing run); a selection that selects
 * nothing.  A corrupt scan ends the call with that message's text; the threads are joined and nothing leaks.
 * Returns out->status: ILCC_OK, ILCC_AMBIGUOUS / ILCC_BOARD_NOT_FOUND of the fusion (per_image_out is complete then), or the
 * failure of a layer below.  out->host_recovery_ms is as in ilcc_bag_corners_all_images. */
int32_t ilcc_bag_corners_all_compressed_images(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera,
                                               int32_t board_w, int32_t board_h, const ilcc_jpeg_sequence_params* sp,
                                               ilcc_image_sequence_result* out, ilcc_image_record* per_image_out, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif
