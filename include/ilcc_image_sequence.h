/*
 * ilcc_image_sequence.h -- camera corners from EVERY image of a recording (in libilcc_hip.so).
 *
 * The reference's get_image_corners_bag stops after the first sensor_msgs/Image of a bag (test/get_image_corners_bag.cpp:78-84),
 * and so do the bag entries of ilcc_camera_image.h.  A calibration bag holds a board that stands still for seconds: tens to
 * hundreds of frames.  The entries here read all of them, detect the corners of a batch of images in at most eight launches
 * (K10b), recover each image's board and fuse the boards into one.  Three layers, each usable alone:
 *
 *   reference                                                     here
 *   ------------------------------------------------------------  -----------------------------------------------------
 *   findCorners.m on one image (ilcc_image_corners.h)              ilcc_image_corners_batch_device on n images (K10b,
 *                                                                   csrc/k10b_image_corners_batch.hip; the stage bodies are
 *                                                                   K10's own, csrc/k10_stages.h)
 *   nonMaximumSuppression.m's scan order (u outer, v inner)        block-id order of the device-side compaction
 *   (none: one detection decides <camera><i>.txt)                  ilcc_fuse_image_corners (host, fp64,
 *                                                                   csrc/image_sequence_host.cpp)
 *   get_image_corners_bag: first Image -> MONO8 -> undistort ->    ilcc_bag_corners_all_images: every selected Image -> K11 ->
 *     imwrite -> MATLAB -> <camera><i>.txt                          K10b -> structure recovery -> fusion
 *                                                                   (csrc/image_sequence_api.cpp)
 *
 * tests/image_sequence_ref.py restates the fusion, the selection and batch cutting and K10b's candidate order in numpy; it
 * is the specification.
 */
#ifndef ILCC_IMAGE_SEQUENCE_H_
#define ILCC_IMAGE_SEQUENCE_H_

#include "ilcc_camera_image.h"
#include "ilcc_hip.h"
#include "ilcc_image_corners.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 1. K10b: findCorners on a batch of images -----------------------------------------------------------------------------
 * All images of a call have one width, height and row stride; image m starts at d_images + m * image_pitch (bytes), and
 * image_pitch >= stride * height.  corners: host, [n_images][capacity]; n_corners: host, [n_images].
 *
 * CONTRACT: for every image m, n_corners[m] and every byte of corners[m][0 .. min(n_corners[m], capacity)) equal what
 * ilcc_image_corners_device returns for that image alone -- both call the same stage bodies, compiled with the same flags, in the
 * same order.  An image with more corners than capacity gets its full count; the call returns ILCC_CAPACITY after EVERY image
 * has been filled up to capacity.  Synchronous on return.
 *
 * The plan owns all scratch: per image the gradients, the likelihood map and one NMS slot per 4 x 4 scan block; per-image min /
 * max; the chunk counts, the compacted candidate list with its per-image offsets, the record buffer, and the page-locked words
 * the counts and records come back through.  It is sized at creation for max_images images of max_width x max_height on the
 * current device; the record buffer may grow, and a growth counts as (two) allocations.  A second call of the same shape
 * allocates nothing.  A plan serves one call at a time; destroy it only after its last call has returned.
 *
 * Launches, each once per batch with the image as a grid dimension: min / max, gradients, likelihood, NMS (each scan block's
 * maximum, or "none", into the block's own slot), count per 256 slots, one workgroup's exclusive prefix, scatter at prefix +
 * rank, refine + score (one wavefront per candidate of the whole batch; the candidate carries its image).  At most EIGHT,
 * whatever n_images is.  The host waits at most twice: for the counts, and for the records; a batch without candidates has no
 * refine launch and one wait.
 *
 * Refusals -- on the host, nothing launched, outputs untouched (ILCC_BAD_ARGUMENT): null pointers, n_images above the plan's
 * limit, an image larger than the plan's, a side below 34 px, stride < width, image_pitch < stride * height, a plan of another
 * device.  n_images == 0 is ILCC_OK with no launch. */
typedef struct ilcc_image_corner_plan ilcc_image_corner_plan;
/* NULL on failure (ilcc_last_error(NULL)); max_images 1 .. 65535, sides 34 .. 65536 */
ilcc_image_corner_plan* ilcc_image_corner_plan_create(uint32_t max_images, int32_t max_width, int32_t max_height);
void ilcc_image_corner_plan_destroy(ilcc_image_corner_plan* plan);
int32_t ilcc_image_corners_batch_device(const void* d_images, uint64_t image_pitch, uint32_t n_images, int32_t width, int32_t height,
                                        int32_t stride, ilcc_image_corner* corners, int32_t capacity, int32_t* n_corners,
                                        ilcc_image_corner_plan* plan, void* hip_stream);
/* kernel launches of the plan's last accepted call (0 .. 8) */
uint32_t ilcc_image_corner_plan_launches(const ilcc_image_corner_plan* plan);
/* device / page-locked allocations made since (and at) creation */
uint32_t ilcc_image_corner_plan_allocations(const ilcc_image_corner_plan* plan);
/* stage output: the compacted NMS maxima of the plan's last accepted call, [image, u, v] (1-based u, v) per candidate in list
 * order, and offsets[0 .. n_images] of each image's part.  ILCC_CAPACITY (offsets filled) when there are more than capacity. */
int32_t ilcc_image_corner_plan_candidates(ilcc_image_corner_plan* plan, int32_t* candidates, uint32_t capacity, uint32_t* offsets);
/* device bytes one image of that size takes in a plan (gradients, map, slots, candidates; each part rounded up to 256); 0 for a
 * size K10b refuses.  Host arithmetic only. */
uint64_t ilcc_image_corner_scratch_bytes(int32_t width, int32_t height);

/* ---- 2. fusion of per-image boards (host, fp64; csrc/image_sequence_host.cpp, plain C++ built with -ffp-contract=off) -------
 * xy: n x (a b) x 2 doubles; image i's part is its board as ilcc_find_chessboard_device gives it: rows[i] x cols[i], row-major,
 * with {rows[i], cols[i]} == {a, b} in either order.  accepted: n flags.
 *   1. S = the accepted images in input order.  S empty: ILCC_BOARD_NOT_FOUND.  ref_image = the first of S; the fused board has
 *      ITS rows x cols (R x C below).
 *   2. every image of S is aligned to ref_image over index variants v: for reference entry (i, j), i2 = (v & 1) ? R - 1 - i : i,
 *      j2 = (v & 2) ? C - 1 - j : j; variants 0-3 read the image's entry (i2, j2) (its shape must be R x C), variants 4-7 its
 *      entry (j2, i2) (its shape must be C x R).  A square board tries all eight.  Cost = the sum over the reference's entries in
 *      index order, then u, v, of the squared fp64 difference, added one by one; a tie goes to the lower variant.
 *   3. m0 = the median per coordinate over S (even count: (lo + hi) / 2).
 *   4. gate: gate_px > 0 is taken as given; otherwise HALF the least distance sqrt(du du + dv dv) between lattice neighbours
 *      ((i, j)-(i+1, j) and (i, j)-(i, j+1)) of m0 -- half a square separates a board from the same board read one square off.
 *      d2_i = max over corners of (du du + dv dv) to m0; image i is USED iff d2_i <= gate gate.
 *   5. n_ok = |S|, n_used = used images.  n_used == 0 or 2 n_used <= n_ok: ILCC_AMBIGUOUS (the board or the camera moved), counts
 *      and rows / cols filled, xy zero.
 *   6. m1 = the same median over the used images = xy (fp64: ilcc_save_cam_corners rounds to %.5g anyway).  spread_max = sqrt of
 *      the largest d2 of a used image to m1; spread_rms = sqrt(sum of all used images' corner distances squared / (n_used a b)).
 * One gating round only.  ILCC_BAD_ARGUMENT: null pointers, a or b < 3, a b > ILCC_MAX_CORNERS, an ACCEPTED image whose shape is
 * neither a x b nor b x a or that holds a non-finite coordinate, a non-finite gate.  Non-accepted images are never read.
 * used_out (n flags) and dist_out (n doubles: sqrt(d2_i) to m1 of every image of S when the status is ILCC_OK, to m0 when it is
 * ILCC_AMBIGUOUS; -1 for images outside S) may be NULL. */
typedef struct ilcc_fused_image_corners {
  int32_t status;
  int32_t n_images, n_ok, n_used;
  int32_t ref_image;             /* -1: none */
  int32_t rows, cols;            /* of the fused board (the reference image's); 0 without one */
  int32_t reserved0;
  double gate;                   /* px: the gate that was applied */
  double spread_rms, spread_max; /* px */
  double xy[ILCC_MAX_CORNERS * 2];
} ilcc_fused_image_corners;
int32_t ilcc_fuse_image_corners(const double* xy, const int32_t* rows, const int32_t* cols, const uint8_t* accepted, uint32_t n,
                                uint32_t a, uint32_t b, double gate_px, ilcc_fused_image_corners* out, uint8_t* used_out,
                                double* dist_out);

/* ---- 3. the chain ---------------------------------------------------------------------------------------------------------- */
typedef struct ilcc_image_sequence_params {
  uint32_t first;               /* first message of the topic that is taken (time order) */
  uint32_t stride;              /* every stride-th from there (0 is read as 1) */
  uint32_t max_images;          /* at most this many (0: all) */
  uint32_t reserved0;           /* the route of structure recovery: 0 ilcc_chessboard_from_corners on a host thread; 1 K18 on the */
                                /*   call's stream right after the batch's K10b (ilcc_image_structure.h): the same records; above 1: */
                                /*   ILCC_BAD_ARGUMENT, refused with the other host-side refusals before anything is allocated */
  double gate_px;               /* <= 0: half a square of the median board (rule 4 above) */
  uint64_t staging_bytes;       /* raw message data per batch; 0: 256 MiB */
  uint64_t device_bytes;        /* mono8 images + K10b scratch per batch; 0: 512 MiB */
} ilcc_image_sequence_params;

typedef struct ilcc_image_record {
  uint32_t message;             /* index of the message on the topic */
  uint32_t stamp_sec, stamp_nsec;   /* the image's header stamp */
  uint32_t time_sec, time_nsec;     /* its record time */
  int32_t status;               /* ILCC_OK / ILCC_BOARD_NOT_FOUND / ILCC_AMBIGUOUS of structure recovery */
  int32_t n_corners;            /* corners K10b found in the image */
  int32_t rows, cols;
  int32_t accepted, used;
  int32_t reserved0;
  double distance;              /* ilcc_fuse_image_corners' dist_out */
  double xy[ILCC_MAX_CORNERS * 2];
} ilcc_image_record;

typedef struct ilcc_image_sequence_result {
  int32_t status;
  int32_t n_images, n_ok, n_used;
  int32_t ref_image;            /* index among the images that ran (per_image_out's index); -1: none */
  int32_t rows, cols;
  int32_t n_batches;
  double gate;
  double spread_rms, spread_max;
  double host_recovery_ms;      /* wall time spent recovering boards, all images, whichever route (reserved0) did it */
  double xy[ILCC_MAX_CORNERS * 2];
} ilcc_image_sequence_result;

void ilcc_default_image_sequence_params(ilcc_image_sequence_params* sp);

/* The batches of a selection, cut before anything is allocated: a batch is as many consecutive images as fit BOTH budgets,
 * raw_bytes[i] rounded up to 256 against staging_bytes and device_bytes_per_image against device_bytes (0: the defaults above).
 * batch_first[0 .. *n_batches] (room for n + 1) gets each batch's first image and n at the end.  One image above a budget:
 * ILCC_CAPACITY.  Host only; what ilcc_bag_corners_all_images cuts with. */
int32_t ilcc_image_sequence_cut(const uint64_t* raw_bytes, uint32_t n, uint64_t device_bytes_per_image, uint64_t staging_bytes,
                                uint64_t device_bytes, uint32_t* batch_first, uint32_t* n_batches);

/* Every selected sensor_msgs/Image of `topic` (the topic iterator of ilcc_sequence.h with the Image md5sum, ilcc_image_parse_any)
 * -> K11 (camera NULL: conversion only) -> K10b -> ilcc_chessboard_from_corners -> ilcc_fuse_image_corners on the images whose
 * status is ILCC_OK.  raw_bytes = the messages' lengths; device_bytes_per_image = width * height rounded up to 256 + ilcc_image_corner_scratch_bytes.  Per batch, on
 * one stream of the call: the raw frames into one page-locked blob at 256-byte aligned offsets, one H2D copy, K11 per image into a
 * packed mono8 array, K10b; the host recovers batch k's boards while the device works on batch k + 1 (two sets of buffers, as
 * large as the largest batch, allocated once per call).
 * CONTRACT: every record's status, rows, cols and xy equal what K11 + ilcc_find_chessboard_device give for that image alone, so
 * record 0 with first = 0 equals ilcc_bag_find_chessboard.
 * Refusals, on the host: a topic with CompressedImage only (ILCC_BAD_ARGUMENT; ilcc_bag_corners_all_compressed_images of
 * ilcc_jpeg_sequence.h takes it); an image of another size or encoding class
 * (mono / colour / Bayer pattern: the encoding itself) than the first selected one, or of another size than camera's
 * (ILCC_BAD_ARGUMENT, the text names the message); an image smaller than K10 takes (ILCC_BAD_ARGUMENT); one image above a budget
 * (ILCC_CAPACITY); per_image_out (cap records; may be NULL with cap 0) smaller than the selection (ILCC_CAPACITY with
 * out->n_images = the number needed, nothing run).
 * Returns out->status: ILCC_OK, ILCC_AMBIGUOUS / ILCC_BOARD_NOT_FOUND of the fusion (per_image_out is complete then), or the
 * failure of a layer below. */
int32_t ilcc_bag_corners_all_images(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera,
                                    int32_t board_w, int32_t board_h, const ilcc_image_sequence_params* sp,
                                    ilcc_image_sequence_result* out, ilcc_image_record* per_image_out, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif
