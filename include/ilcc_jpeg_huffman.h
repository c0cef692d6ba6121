/*
 * ilcc_jpeg_huffman.h -- K16: the Huffman scans of a batch of JPEG frames decoded on the GPU (in libilcc_hip.so).
 *
 * ilcc_jpeg_entropy_decode walks a scan bit by bit on one host core; K16 does the same work on the device, so that a chain can
 * stage a frame's file bytes instead of its coefficients.  Sequential Huffman data has no random access; the method is
 * self-synchronising subsequence decoding (Weissenberger and Schmidt, "Massively Parallel Huffman Decoding on GPUs", ICPP
 * 2018): the bits are cut into subsequences, every subsequence is decoded from a guessed state, and is decoded again from its
 * left neighbour's exit state until no exit state changes.  A camera frame settles in two or three rounds; a flat image never
 * does, and is right only because the number of rounds is bounded by the number of subsequences.
 *
 *   host (ilcc_jpeg.h)                                            here
 *   ------------------------------------------------------------  -----------------------------------------------------------
 *   Bits::fill of csrc/jpeg_entropy.cpp: unstuffing and RSTn      ilcc_jpeg_scan_prepare (csrc/jpeg_scan_prepare.cpp, plain C++
 *     while the bits are decoded                                    without HIP): one pass over the bytes, no Huffman decoding
 *   ilcc_jpeg_entropy_decode on one image                         ilcc_jpeg_huffman_batch_device on n images of one geometry
 *                                                                   (K16, csrc/k16_jpeg_huffman.hip); its output is K13b's input
 */
#ifndef ILCC_JPEG_HUFFMAN_H_
#define ILCC_JPEG_HUFFMAN_H_

#include <stdint.h>

#include "ilcc_jpeg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One restart interval of a scan (or the whole scan of a file without restart markers).  It starts on a byte boundary. */
typedef struct ilcc_jpeg_huffman_segment {
  uint32_t byte_offset;         /* into the image's unstuffed scan */
  uint32_t byte_count;
  uint32_t first_mcu;           /* in scan order */
  uint32_t mcu_count;
} ilcc_jpeg_huffman_segment;    /* 16 bytes */

/* One Huffman table as the kernel reads it, field for field what the host decoder builds from a DHT segment. */
typedef struct ilcc_jpeg_huffman_table {
  uint16_t look[512];           /* 9-bit prefix -> length << 8 | symbol, 0: the code is longer than 9 bits */
  int32_t maxcode[17];          /* largest code of each length 1 .. 16, -1: none; [0] is 0 */
  int32_t first[17];            /* index in values[] of the first code of each length, minus that code; [0] is 0 */
  uint8_t values[256];          /* the symbols in code order; 0 behind the last one */
} ilcc_jpeg_huffman_table;      /* 1416 bytes */

/* The tables of one image's scan by COMPONENT (not by table index): component c decodes with dc[c] and ac[c].  Components the
 * image does not have are all zero. */
typedef struct ilcc_jpeg_huffman_tables {
  ilcc_jpeg_huffman_table dc[3], ac[3];
} ilcc_jpeg_huffman_tables;     /* 8496 bytes */

/* Where one image of a batch lies in the batch's concatenated arrays. */
typedef struct ilcc_jpeg_huffman_image {
  uint64_t scan_offset;         /* of the image's unstuffed scan in d_scans, bytes */
  uint32_t scan_bytes;
  uint32_t first_segment;       /* row of d_segments */
  uint32_t n_segments;
  uint32_t reserved;
} ilcc_jpeg_huffman_image;      /* 24 bytes */

/* What K16 leaves in its scratch, one per image, once the stream has run: how the synchronisation went.  A chunk is up to 256
 * consecutive subsequences of a segment; a round is one pass in which the subsequences whose entry state changed are decoded
 * again. */
typedef struct ilcc_jpeg_huffman_counters {
  uint32_t subsequences;
  uint32_t chunks;
  uint32_t rounds;              /* summed over the chunks */
  uint32_t max_rounds;          /* of one chunk */
} ilcc_jpeg_huffman_counters;   /* 16 bytes */

/* bits of ilcc_jpeg_huffman_batch_device's d_status[m]; 0: the image's coefficients are the host decoder's */
#define ILCC_JPEG_HUFFMAN_NO_CODE      0x01u   /* a Huffman code in no table */
#define ILCC_JPEG_HUFFMAN_RUN_PAST_63  0x02u   /* a run past coefficient 63 */
#define ILCC_JPEG_HUFFMAN_DC_CATEGORY  0x04u   /* a DC difference category above 15 */
#define ILCC_JPEG_HUFFMAN_DC_RANGE     0x08u   /* a DC predictor that leaves int16 */
#define ILCC_JPEG_HUFFMAN_ENDS_EARLY   0x10u   /* the bits of a segment end before its blocks do */
#define ILCC_JPEG_HUFFMAN_BAD_ROWS     0x20u   /* an image or segment row that points outside the arrays or the image */

/* ---- 1. the host's part: unstuffing, restart markers, tables -----------------------------------------------------------------
 * Upper bounds of what ilcc_jpeg_scan_prepare writes for a file of `file_bytes` bytes whose headers gave `info`: the unstuffed
 * scan is never longer than the bytes behind the headers, and there is one segment per restart interval.  ILCC_BAD_ARGUMENT: null
 * pointers, an info ilcc_jpeg_layout would not make, a scan_offset behind the file's end. */
int32_t ilcc_jpeg_scan_bound(const ilcc_jpeg_info* info, uint64_t file_bytes, uint64_t* scan_bytes, uint32_t* n_segments);

/* `jpg` and the `info` ilcc_jpeg_parse made of it -> the unstuffed entropy-coded bytes of the scan in scan[0 .. *scan_bytes), its
 * segments[0 .. *n_segments) and *tables.  Any run of 0xFF followed by 0x00 is the data byte 0xFF; a run followed by RSTn ends
 * a segment; a run followed by anything else, or by nothing, ends the scan, as in the host decoder.  No Huffman code is decoded:
 * what ilcc_jpeg_entropy_decode refuses INSIDE the bits, K16 reports per image.  Everything else the host decoder refuses is
 * refused here, for the same causes and in the same words: headers that do not parse, an info that is not these bytes', a
 * restart marker missing or out of order, several scans, DNL.  ILCC_CAPACITY: scan_cap or segment_cap too small (the bound above
 * never is), or a scan of 2^28 bytes or more.  Allocates nothing; never reads past `bytes`.  Host only. */
int32_t ilcc_jpeg_scan_prepare(const uint8_t* jpg, uint64_t bytes, const ilcc_jpeg_info* info, uint8_t* scan, uint64_t scan_cap,
                               uint64_t* scan_bytes, ilcc_jpeg_huffman_segment* segments, uint32_t segment_cap, uint32_t* n_segments,
                               ilcc_jpeg_huffman_tables* tables);

/* ---- 2. K16 ------------------------------------------------------------------------------------------------------------------
 * The entry takes ONE struct, not a parameter list: a dozen arguments are easier to name than to order, and the project's test
 * that every declaration with a stream argument has a delayed-stream case reads parameter lists (K16's delayed-stream cases are in
 * tests/test_jpeg_huffman.py).
 *
 * layout     geometry shared by the batch, as for K13b: n_components, h / v, blocks_w / blocks_h, coef_offset, coef_count.
 * d_scans    the images' unstuffed scans, concatenated (scans_bytes in all); no alignment asked.
 * d_tables   [n_images] ilcc_jpeg_huffman_tables, 16-byte aligned.
 * d_segments [n_segments] rows, 16-byte aligned; image m's are rows first_segment .. first_segment + n_segments - 1.
 * d_images   [n_images] rows, 8-byte aligned.
 * d_coef     image m's coefficients at d_coef + m * coef_pitch (int16 units; >= coef_count, a multiple of 8), 16-byte aligned:
 *            K13b's input.
 * d_status   [n_images] uint32.
 * d_scratch  ilcc_jpeg_huffman_scratch_bytes(n_images) bytes, 16-byte aligned: [n_images] ilcc_jpeg_huffman_counters when the
 *            stream has run.  It belongs to the call until then.
 * max_segments  the largest n_segments of any image of the batch (the grid's width).
 * subsequence_bits  S: 256, 512, 1024 or 2048; 0: ILCC_JPEG_HUFFMAN_DEFAULT_BITS.
 *
 * CONTRACT on coefficients: for every image the host decoder accepts, d_status[m] == 0 and all coef_count int16 of image m equal
 * ilcc_jpeg_entropy_decode's byte for byte, the blocks that pad the image to whole MCUs and the zeros included; the int16
 * between coef_count and coef_pitch are not written.
 * CONTRACT on status: for every image the host decoder refuses inside the scan, d_status[m] != 0 (the bits above).  Its
 * coefficients are unspecified, nothing is written outside its own coef_count int16 whatever the bits, the rows and the tables say,
 * and the other images of the batch are what they would be without it.
 * Asynchronous on hip_stream, no allocation, no host wait; *job is read before the call returns.  n_images == 0: ILCC_OK, no
 * launch.
 *
 * THREE launches, whatever n_images is.  No workgroup waits for another, nothing spins on memory, no cooperative launch; every
 * loop is bounded and every step of a decoder consumes at least one bit, so garbage terminates.
 *   k16_clear   zeroes the coefficients, d_status and the counters.
 *   k16_decode  one workgroup of 256 threads per segment, grid (max_segments, n_images); the image's tables are staged in LDS once,
 *               and each chunk's bytes (256 * S / 8: 64 KB at S = 2048, dynamic LDS) before its passes read them.
 *               The segment is cut into subsequences of S bits and walked in chunks of 256 subsequences; the exact exit state of
 *               a chunk is the entry state of the next.  A decoder state is (bit position, block inside the MCU, coefficient
 *               index with 0 = a DC code comes next).  Per chunk:
 *                 cold pass   thread i decodes subsequence i from (its first bit, block 0, DC) -- the chunk's first one from the
 *                             exact state -- to the first symbol boundary at or behind its end; a symbol is a code with its
 *                             extra bits.  Exit states go to LDS.
 *                 rounds      thread i takes thread i - 1's exit of the round before; where that differs from what it last
 *                             started from it decodes again.  The rounds end when no exit changed, after at most (subsequences of
 *                             the chunk) - 1 of them: subsequence i is exact after round i.
 *                 count       the blocks each subsequence completes come out of its last decode; an exclusive prefix sum places
 *                             them.
 *                 write       every thread decodes once more from its exact state and stores each coefficient at
 *                             coef_offset_c + (by * blocks_w_c + bx) * 64 + zigzag[k], the DC as the DIFFERENCE, stops at the
 *                             segment's block count and reports what the host decoder refuses.
 *               While a state is a guess nothing is an error: a code in no table skips one bit, a run past coefficient 63 closes
 *               the block, a DC category above 15 is a difference of 0 without extra bits, bits that end clamp the position to
 *               the segment's end.  The count uses the same rules, so it agrees with the write pass up to the first refusal.
 *   k16_dc      one workgroup per (segment, component): an inclusive prefix sum of the component's DC differences in scan order,
 *               256 blocks at a time, int32 with the int16 range check, stored over the differences. */
#define ILCC_JPEG_HUFFMAN_DEFAULT_BITS 2048u   /* measured: DESIGN section 9 */

typedef struct ilcc_jpeg_huffman_job {
  const ilcc_jpeg_info* layout;
  const uint8_t* d_scans;
  uint64_t scans_bytes;
  const ilcc_jpeg_huffman_tables* d_tables;
  const ilcc_jpeg_huffman_segment* d_segments;
  const ilcc_jpeg_huffman_image* d_images;
  int16_t* d_coef;
  uint64_t coef_pitch;
  uint32_t* d_status;
  void* d_scratch;
  uint64_t scratch_bytes;
  uint32_t n_images;
  uint32_t n_segments;          /* rows of d_segments */
  uint32_t max_segments;
  uint32_t subsequence_bits;
  void* hip_stream;
} ilcc_jpeg_huffman_job;        /* 112 bytes */

uint64_t ilcc_jpeg_huffman_scratch_bytes(uint32_t n_images);

/* Refusals -- on the host, nothing launched (ILCC_BAD_ARGUMENT): a null job or pointer, a layout ilcc_jpeg_layout would not make,
 * n_images above 65535, a coef_pitch short of coef_count or not a multiple of 8, a misaligned d_coef, d_tables, d_segments,
 * d_images, d_status or d_scratch, too little scratch, max_segments of 0 or above n_segments, a subsequence_bits outside the
 * accepted set. */
int32_t ilcc_jpeg_huffman_batch_device(const ilcc_jpeg_huffman_job* job);

/* ---- 3. in the chain ----------------------------------------------------------------------------------------------------------
 * ilcc_bag_corners_all_compressed_images (ilcc_jpeg_sequence.h) decodes with K16 when ilcc_jpeg_sequence_params.reserved0 is 1: per
 * batch the pool's threads run only ilcc_jpeg_scan_prepare into the page-locked blob, ONE H2D copy moves scans, tables and rows,
 * then K16, K13b and onwards as on the host route; the statuses travel back behind K16 and are read after K10b's wait, before
 * structure recovery, and an image K16 flags is decoded once by
 * ilcc_jpeg_entropy_decode, whose status and text end the call as they end the host route.  (Should the host decoder accept what
 * K16 flagged, the call ends with ILCC_HIP_ERROR and a text that says "internal error".)  The records do not depend on the route.
 *
 * What one image of `layout` whose file has data_bytes bytes and n_segments restart intervals takes on that route; with up(x) = x
 * rounded up to 256:
 *   staged = up(data_bytes) + up(8496) + up(2 * 3 * 64) + up(24) + up(16 * n_segments)
 *                                                        the file's bytes bound its unstuffed scan; tables; quantisation rows;
 *                                                        image row; segment rows: what the H2D copy moves
 *   device = staged + up(2 * coef_count) + 512           the coefficients K16 writes; its status and counters
 *                   + the planes, pixels, mono8 and K10b parts of ilcc_jpeg_sequence_bytes
 * The chain cuts its batches with each image's own `staged` against staging_bytes and the largest `device` of the selection
 * against device_bytes.  ILCC_BAD_ARGUMENT: null pointers, a layout ilcc_jpeg_layout would not make. */
int32_t ilcc_jpeg_huffman_sequence_bytes(const ilcc_jpeg_info* layout, uint64_t data_bytes, uint32_t n_segments, uint64_t* staged_bytes,
                                         uint64_t* device_bytes);

#ifdef __cplusplus
}
#endif
#endif
