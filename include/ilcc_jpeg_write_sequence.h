/*
 * ilcc_jpeg_write_sequence.h -- writing EVERY undistorted frame of a recording as <prefix><i>.jpg (in libilcc_hip.so).
 *
 * ilcc_jpeg_write.h writes one image per call: one allocation, the whole coefficient array copied to the host, one serial
 * Huffman pass on one host core.  The entries here are the batch path, the mirror of ilcc_jpeg_sequence.h and
 * ilcc_jpeg_huffman.h on the writing side: the coefficients never leave the device, what comes back is the scans.  Four
 * layers, each usable alone:
 *
 *   single image (ilcc_jpeg_write.h)                              here
 *   ------------------------------------------------------------  -----------------------------------------------------------
 *   write_headers inside ilcc_jpeg_entropy_encode                 ilcc_jpeg_write_headers: SOI .. SOS header (host,
 *                                                                   csrc/jpeg_entropy_enc.cpp); a file is headers + scan + FF D9
 *   ilcc_jpeg_fdct_device on one image (K14)                      ilcc_jpeg_fdct_batch_device on n images (K14b,
 *                                                                   csrc/k14b_jpeg_write_batch.hip; the stage bodies are K14's
 *                                                                   own, csrc/k14_stages.h)
 *   the scan loop of ilcc_jpeg_entropy_encode on one host core    ilcc_jpeg_huffman_encode_batch_device on n images (K17,
 *                                                                   csrc/k17_jpeg_huffman_enc.hip)
 *   ilcc_bag_save_jpeg: the first frame                           ilcc_bag_save_jpeg_all: every selected one
 *                                                                   (csrc/jpeg_write_sequence_api.cpp)
 *
 * tests/jpeg_huffman_enc_ref.py restates K17's steps in numpy; it is the specification.
 */
#ifndef ILCC_JPEG_WRITE_SEQUENCE_H_
#define ILCC_JPEG_WRITE_SEQUENCE_H_

#include <stdint.h>

#include "ilcc_camera_image.h"
#include "ilcc_jpeg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 1. the bytes around the scan (host) ---------------------------------------------------------------------------------------
 * Exactly what ilcc_jpeg_entropy_encode writes in front of the scan, by the same function: SOI, APP0, DQT, SOF0, DHT, DRI when the
 * interval is non-zero, and the SOS header.  *bytes is their count (at most 629).  Allocates nothing, writes nothing past `cap`
 * (ILCC_CAPACITY).  ILCC_BAD_ARGUMENT: null pointers, an info that is not ilcc_jpeg_write_info's shape.  Host only. */
int32_t ilcc_jpeg_write_headers(const ilcc_jpeg_info* info, uint8_t* out, uint64_t cap, uint64_t* bytes);

/* ---- 2. K14b: colour conversion, downsampling, forward DCT and quantisation on a batch ------------------------------------------
 * n images of one geometry and one set of quantisation tables (`layout`: an info of ilcc_jpeg_write_info's shape).  Image m lies at
 * d_src + m * image_pitch (bytes; >= src_stride * (height - 1) + a row), rows src_stride apart, ILCC_ENCODING_MONO8 for 1
 * component and ILCC_ENCODING_BGR8 for 3.  Its coefficients go to d_coef + m * coef_pitch (int16 units; >= coef_count, a multiple
 * of 8), d_coef 16-byte aligned.  d_scratch (3 components only): ilcc_jpeg_fdct_batch_scratch_bytes bytes, 16-byte aligned; image
 * m's three padded planes at d_scratch + m * ilcc_jpeg_fdct_scratch_bytes(layout).
 * CONTRACT: every image's coef_count int16 equal ilcc_jpeg_fdct_device's for that image alone, byte for byte, dummy blocks
 * included; nothing is written between coef_count and coef_pitch.  Asynchronous on hip_stream, no allocation, no host wait; *job and
 * *layout are read before the call returns.  n_images == 0: ILCC_OK, no launch.
 *
 * Launches, whatever n_images is: for 3 components ONE k14b_colour_downsample with the image as blockIdx.z, then ONE k14b_fdct_quant
 * for all components of all images (the image is blockIdx.z, (component, block row) is flattened into blockIdx.y as in K13b,
 * blockIdx.x is the 32-block group sized for luma).  Two launches per colour batch, one per gray batch.
 *
 * Refusals -- on the host, nothing launched (ILCC_BAD_ARGUMENT): a null job or pointer, a layout ilcc_jpeg_layout would not make
 * or with a quantisation entry outside 1 .. 255, an encoding that does not fit the components, n_images above 65535, a src_stride
 * shorter than a row, an image_pitch short of an image, a coef_pitch short of coef_count or not a multiple of 8, a misaligned
 * d_coef or d_scratch, too little scratch. */
typedef struct ilcc_jpeg_fdct_batch_job {
  const ilcc_jpeg_info* layout;
  const void* d_src;
  uint64_t image_pitch;
  int32_t src_stride;
  int32_t encoding;
  int16_t* d_coef;
  uint64_t coef_pitch;
  void* d_scratch;
  uint64_t scratch_bytes;
  uint32_t n_images;
  uint32_t reserved;
  void* hip_stream;
} ilcc_jpeg_fdct_batch_job;     /* 80 bytes */

uint64_t ilcc_jpeg_fdct_batch_scratch_bytes(const ilcc_jpeg_info* layout, uint32_t n_images);   /* 0 for 1 component / a refused layout */
int32_t  ilcc_jpeg_fdct_batch_device(const ilcc_jpeg_fdct_batch_job* job);

/* ---- 3. K17: the Huffman scans of a batch -----------------------------------------------------------------------------------------
 * Every block's bit length follows from its own coefficients and the preceding DC of its component, so nothing has to
 * synchronise itself: lengths, prefix sums, and every block writes its codes at its own bit offset.
 *
 * layout     geometry shared by the batch, an info of ilcc_jpeg_write_info's shape: table indices 0 / 1 (the Annex-K tables),
 *            restart interval 0 .. 65535.  Its quant[] is NOT read.
 * d_coef     image m's coefficients at d_coef + m * coef_pitch (int16 units; >= coef_count, a multiple of 8), 16-byte aligned: what
 *            K14b leaves.
 * d_out      out_cap bytes for the whole batch, 16-byte aligned.
 * d_rows     [n_images] rows, 8-byte aligned: where image m's scan lies in d_out, and its status.
 * d_scratch  ilcc_jpeg_huffman_encode_scratch_bytes(layout, n_images, out_cap) bytes, 256-byte aligned.  It belongs to the call until
 *            the stream has run.
 *
 * CONTRACT on bytes: for every image whose coefficients ilcc_jpeg_entropy_encode accepts and that fits, d_rows[m].status == 0 and
 * d_out[offset .. offset + bytes) equals ilcc_jpeg_entropy_encode's file from the first byte behind its SOS header up to, but not
 * including, its EOI: the stuffed data, the 1-bit padding before every RSTn and at the end, RSTn every restart_interval MCUs
 * with the counter wrapping at 8.  Byte for byte.  Images are placed in order at 16-byte aligned offsets; the bytes between them
 * are not written.
 * CONTRACT on refusals: a DC difference outside 11 bits or an AC value outside 10 bits (what the host encoder refuses) sets the
 * image's bit below; the image takes 0 bytes and the images behind it are what they would be without it.  If an image's end
 * lies past out_cap, that image and every image behind it get ILCC_JPEG_ENCODE_CAPACITY and 0 bytes.  Nothing is ever written
 * at or past d_out + out_cap, whatever the coefficients say.
 * Asynchronous on hip_stream, no allocation, no host wait; *job and *layout are read before the call returns.  n_images == 0:
 * ILCC_OK, no launch.
 *
 * EIGHT launches, whatever n_images and the coefficients are.  No workgroup waits for another, nothing spins on memory, no
 * cooperative launch; every loop is bounded by a count the host knows.  With B = coef_count / 64 blocks an image in scan order, a
 * TILE of 256 consecutive blocks, a SEGMENT = one restart interval (restart_interval MCUs; the whole scan without one), and the
 * UNSTUFFED buffer in the scratch, where image m's scan lies on a 4096-byte boundary as segments on byte boundaries, each but
 * the last followed by a hole of two zero bytes where its RSTn will go:
 *   k17_clear           zeroes the unstuffed buffer.
 *   k17_count           one thread per block, grid (tiles, n_images): the DC difference against the previous block of the same
 *                       component in scan order (predictor 0 at a segment's start; index arithmetic, no state), the block's bit
 *                       count from the Annex-K code lengths (staged in LDS), the two range checks; an exclusive prefix of the
 *                       counts inside the tile, and the tile's sum with the refusal bits.
 *   k17_layout          one workgroup per image: the exclusive prefix of the tile sums (256 at a time with a carry); then for
 *                       every segment its bits = the difference of two prefixes, its bytes = ceil(bits / 8) + 2 for the marker
 *                       (not behind the last), and their exclusive prefix: the segment's byte offset in the image's unstuffed
 *                       scan, and the scan's length.  A refused image has length 0.
 *   k17_place_unstuffed one workgroup: the images' offsets in the unstuffed buffer, a prefix over the batch.  The buffer holds
 *                       out_cap + 4096 n_images bytes, which suffices whenever the output fits, since a scan is never longer
 *                       stuffed than unstuffed; an image that does not fit there can not fit in d_out either and is left out,
 *                       with every image behind it.
 *   k17_pack            one thread per block: its codes at (segment's byte offset) * 8 + (block's bit offset in the segment), as
 *                       big-endian 32-bit words.  A word that the block covers whole is a plain store; its first and last word
 *                       may be shared with neighbours (a 4:2:0 chroma block of zeros is 4 bits: eight blocks share one word)
 *                       and are ORed in atomically, which commutes.  A segment's last block appends the 1-bits up to the byte
 *                       boundary.
 *   k17_count_ff        one workgroup per 4096 bytes of the unstuffed buffer, 16 bytes a thread: the 0xFF bytes of each 16, their
 *                       exclusive prefix inside the 4096 and the sum.  Holes and gaps are zero and count nothing.
 *   k17_place           one workgroup: the prefix of those sums; each image's stuffed size = unstuffed + its 0xFF bytes; the
 *                       offsets in d_out, a prefix over the batch of the sizes rounded up to 16; the capacity rule; d_rows.
 *   k17_stuff           one workgroup per 4096 unstuffed bytes: every byte goes to index + (0xFF bytes before it in the image), a
 *                       0x00 behind each 0xFF; the two bytes of a hole become FF, D0 + (segment & 7).  The image of a chunk and
 *                       the segment of a thread's first byte are found by binary search.
 * Not a launch of its own: RSTn markers (k17_stuff writes them, so no second writer ever meets the hole). */
#define ILCC_JPEG_ENCODE_DC_RANGE  0x01u   /* a DC difference outside 11 bits */
#define ILCC_JPEG_ENCODE_AC_RANGE  0x02u   /* an AC value outside 10 bits */
#define ILCC_JPEG_ENCODE_CAPACITY  0x04u   /* the image's end, or the end of an image in front of it, lies past out_cap */

typedef struct ilcc_jpeg_encode_row {
  uint64_t offset;              /* of the image's scan in d_out, a multiple of 16 */
  uint32_t bytes;               /* 0 when status != 0 */
  uint32_t status;
} ilcc_jpeg_encode_row;         /* 16 bytes */

typedef struct ilcc_jpeg_huffman_encode_job {
  const ilcc_jpeg_info* layout;
  const int16_t* d_coef;
  uint64_t coef_pitch;
  uint8_t* d_out;
  uint64_t out_cap;
  ilcc_jpeg_encode_row* d_rows;
  void* d_scratch;
  uint64_t scratch_bytes;
  uint32_t n_images;
  uint32_t reserved;
  void* hip_stream;
} ilcc_jpeg_huffman_encode_job; /* 80 bytes */

/* 0 for a layout the entry refuses */
uint64_t ilcc_jpeg_huffman_encode_scratch_bytes(const ilcc_jpeg_info* layout, uint32_t n_images, uint64_t out_cap);

/* Refusals -- on the host, nothing launched (ILCC_BAD_ARGUMENT): a null job or pointer, a layout ilcc_jpeg_layout would not make or
 * with table indices outside 0 / 1 or a restart interval outside 0 .. 65535, a layout of so many blocks that an image's worst-case
 * scan has 2^32 bits or more, n_images above 65535, out_cap of 2^40 or more, a coef_pitch short of coef_count or not a multiple of
 * 8, a misaligned d_coef, d_out, d_rows or d_scratch, too little scratch. */
int32_t ilcc_jpeg_huffman_encode_batch_device(const ilcc_jpeg_huffman_encode_job* job);

/* ---- 4. the chain ------------------------------------------------------------------------------------------------------------- */
typedef struct ilcc_jpeg_write_sequence_params {
  uint32_t first;               /* first message of the topic that is taken (time order) */
  uint32_t stride;              /* every stride-th from there (0 is read as 1) */
  uint32_t max_images;          /* at most this many (0: all) */
  uint32_t route;               /* 0: K17.  1: the single-image way per image: the coefficients device to host, then
                                 * ilcc_jpeg_entropy_encode.  Anything else: ILCC_BAD_ARGUMENT.  The files do not depend on it. */
  uint64_t staging_bytes;       /* raw message data per batch; 0: 256 MiB */
  uint64_t device_bytes;        /* device bytes per batch (ilcc_jpeg_write_sequence_bytes per image); 0: 512 MiB */
  uint64_t out_bytes_per_image; /* room in K17's output per image of a batch; 0: width * height */
} ilcc_jpeg_write_sequence_params;   /* 40 bytes */

typedef struct ilcc_jpeg_write_record {
  uint32_t message;             /* index of the message on the topic: the file is <prefix><message, 6 digits>.jpg */
  uint32_t stamp_sec, stamp_nsec;   /* the image's header stamp */
  uint32_t time_sec, time_nsec;     /* its record time */
  uint32_t route;               /* the route THIS image took: 0 K17, 1 the host encoder (asked for, or the capacity fallback) */
  uint64_t file_bytes;
} ilcc_jpeg_write_record;       /* 32 bytes */

typedef struct ilcc_jpeg_write_sequence_result {
  int32_t status;
  int32_t n_images;
  int32_t n_batches;
  int32_t n_host_encoded;       /* images that took route 1 */
  uint64_t d2h_bytes;           /* device-to-host bytes of the call: rows and scans, or coefficients */
  uint64_t file_bytes;          /* sum over the files */
} ilcc_jpeg_write_sequence_result;   /* 32 bytes */

void ilcc_default_jpeg_write_sequence_params(ilcc_jpeg_write_sequence_params* sp);

/* device bytes one mono8 image of that size takes in the chain, with up(x) = x rounded up to 256 (host arithmetic; what the chain
 * cuts its batches with, beside the messages' lengths against staging_bytes):
 *   up(width * height)                 mono8 behind K11
 *   + up(2 * coef_count)               K14b's coefficients
 *   + up(out) + 256                    K17's output, out = out_bytes_per_image (0: width * height) rounded up to 16; the image's row
 *   + ilcc_jpeg_huffman_encode_scratch_bytes(layout, 1, out)   K17's scratch for one image; a batch's is never more than its images' sum
 * A CompressedImage topic adds, per image, what its decode takes in ilcc_jpeg_sequence.h: K13b's planes and the decoded pixels.
 * 0 for a size the writer refuses. */
uint64_t ilcc_jpeg_write_sequence_bytes(int32_t width, int32_t height, uint64_t out_bytes_per_image);

/* Every selected sensor_msgs/Image of `topic` (or, when it carries none, every selected sensor_msgs/CompressedImage, decoded as
 * ilcc_bag_save_jpeg decodes the first) -> K11 per image (mono8, undistorted with `camera`; NULL: conversion only) into a packed
 * array -> K14b -> K17 -> device to host: the rows, then ONE copy of the scans actually produced -> one file per image,
 * "%s%06u.jpg" of (path_prefix, message index) = headers + scan + FF D9.  Selection as in ilcc_image_sequence.h; the batches are cut
 * with ilcc_image_sequence_cut from the messages' lengths and ilcc_jpeg_write_sequence_bytes before anything is allocated; the
 * buffers are allocated once per call and sized by the largest batch.  An image K17 flags with ILCC_JPEG_ENCODE_CAPACITY is finished
 * on route 1 from its coefficients; a range refusal ends the call with the host encoder's status and text, the message named.
 * CONTRACT: every file equals, byte for byte, what ilcc_bag_save_jpeg writes for that message alone; the files do not depend on
 * `route` or on how the batches were cut.
 * Refusals, on the host: null bag_path / topic / path_prefix / sp / out; a route above 1; an image of another size or encoding
 * than the first selected one, or of another size than camera's (ILCC_BAD_ARGUMENT, the text names the message); one image above
 * a budget (ILCC_CAPACITY); records (cap of them; may be NULL with cap 0) fewer than the selection (ILCC_CAPACITY with
 * out->n_images = the number needed, nothing run).  Returns out->status. */
int32_t ilcc_bag_save_jpeg_all(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera,
                               const char* path_prefix, int32_t quality, const ilcc_jpeg_write_sequence_params* sp,
                               ilcc_jpeg_write_sequence_result* out, ilcc_jpeg_write_record* records, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif
