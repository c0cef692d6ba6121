/*
 * ilcc_image_structure.h -- chessboardsFromCorners on a BATCH of corner lists, on the GPU (K18; in libilcc_hip.so).
 *
 * ilcc_chessboard_from_corners (ilcc_image_corners.h) regrows the whole board from every seed corner on one host thread, and every
 * growth step rebuilds a candidates x predictions distance matrix four times: a cluttered frame with a thousand corners costs the
 * host a tenth of a second, a 16 x 16 lattice a second.  A seed's board depends on the image's corner list and the seed alone, so
 * K18 grows every (image, seed) pair on a wavefront of its own and leaves only the overlap rule sequential.
 *
 *   reference                                                     here (csrc/k18_chessboard_structure.hip)
 *   ------------------------------------------------------------  -----------------------------------------------------
 *   initChessboard.m, growChessboard.m, chessboardEnergy.m and     k18_grow: one wavefront per (image, seed corner); the
 *     the grow loop of chessboardsFromCorners.m, per seed            image's positions staged once per workgroup in LDS
 *   chessboardsFromCorners.m: keep below -10, the overlap rule,    k18_select: one workgroup per image, seeds in corner
 *     then the one board of the requested shape                      order, an owner[corner] array in LDS
 *
 * TWO launches per call, whatever the batch holds.  The tie rules of the host code are part of the contract: the first minimum in
 * ascending corner index (directionalNeighbor), the first minimum in column-major order of the distance matrix
 * (assignClosestCorners), the lowest border among equal proposals; every fp64 expression keeps the host's operation order, so
 * energies and initChessboard's distances are bit for bit the host's.  Only predictCorners' atan2 / cos / sin differ from glibc in
 * the last bit; they feed an arg-min alone.
 *
 * Device capacities.  An image above one of them, or one that meets a loop bound, is MARKED and recomputed by
 * ilcc_chessboard_from_corners on the host after the device has returned: the result is the host's whatever happens, and the plan
 * counts such images.  Marking is conservative: a seed whose PROPOSAL would exceed a board capacity marks its image.
 */
#ifndef ILCC_IMAGE_STRUCTURE_H_
#define ILCC_IMAGE_STRUCTURE_H_

#include "ilcc_hip.h"
#include "ilcc_image_corners.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ILCC_STRUCTURE_MAX_CORNERS 4096 /* corners of one image on the device path (64 KB of LDS, one "used" bit per lane and word) */
#define ILCC_STRUCTURE_MAX_CELLS ILCC_MAX_CORNERS /* cells of a grown board: 256 */
#define ILCC_STRUCTURE_MAX_SIDE 64      /* rows or columns of a grown board: one prediction per lane */
#define ILCC_STRUCTURE_MAX_ABS 1e15     /* |u|, |v| and the direction components: finite, and squares that cannot overflow */

typedef struct ilcc_structure_plan ilcc_structure_plan;

/* All scratch for calls of up to max_images images with up to max_corners_per_image corners each, on the current device: one
 * device and one page-locked allocation.  max_images 1 .. 65535, max_corners_per_image >= 1 (images above
 * ILCC_STRUCTURE_MAX_CORNERS are accepted and recomputed on the host).  NULL on failure (ilcc_last_error(NULL)).  A plan serves
 * one call at a time; destroy it only after its last call has returned. */
ilcc_structure_plan* ilcc_structure_plan_create(uint32_t max_images, uint32_t max_corners_per_image);
void ilcc_structure_plan_destroy(ilcc_structure_plan* plan);

/* corners: host, [n_images][capacity] with n_corners[n_images] valid entries each -- exactly what ilcc_image_corners_batch_device
 * returns.  status / rows / cols: host, [n_images]; board_index: host, [n_images][board_w * board_h].
 * CONTRACT: for every image, status, rows, cols and board_index equal what ilcc_chessboard_from_corners gives for that image alone
 * (board_index of an image without ILCC_OK is left as it was), whatever the batch holds around it.  Per-image failures
 * (ILCC_BOARD_NOT_FOUND, ILCC_AMBIGUOUS) go into status[]; the return value is ILCC_OK unless the call itself was refused or a HIP
 * call failed.  Synchronous on return; copies and launches on `stream` (hipStream_t or NULL).  The parameter is not called
 * hip_stream: tests/stream_contract.py takes every declaration with a parameter of that name through its late-producer scheme, which
 * needs a device input that a delayed stream can still be writing, and this entry reads and writes host memory only;
 * tests/test_image_structure.py runs it on side streams instead.
 * Refusals -- on the host, nothing launched, outputs untouched (ILCC_BAD_ARGUMENT): null pointers (a null plan among them), a side
 * below 3, board_w * board_h > ILCC_MAX_CORNERS, a negative count or capacity, capacity below an image's n_corners, n_images or a
 * corner count above the plan's, a plan of another device.  n_images == 0 is ILCC_OK with no launch. */
int32_t ilcc_chessboards_from_corners_batch(const ilcc_image_corner* corners, int32_t capacity, const int32_t* n_corners,
                                            uint32_t n_images, int32_t board_w, int32_t board_h, int32_t* status, int32_t* rows,
                                            int32_t* cols, int32_t* board_index, ilcc_structure_plan* plan, void* stream);

/* kernel launches of the plan's last accepted call (0 or 2) */
uint32_t ilcc_structure_plan_launches(const ilcc_structure_plan* plan);
/* images of the last accepted call that the host recomputed */
uint32_t ilcc_structure_plan_fallbacks(const ilcc_structure_plan* plan);
/* device / page-locked allocations since (and at) creation */
uint32_t ilcc_structure_plan_allocations(const ilcc_structure_plan* plan);

/* stage output of the plan's last accepted call: the board that `seed` of `image` grew to BEFORE the keep-below--10 test and the
 * overlap rule, as *rows x *cols corner indices (row-major) in index[cap], and its energy.  *rows == 0: the seed has no board
 * (initChessboard rejected it, or its 3 x 3 board has an energy above 0).  ILCC_CAPACITY: cap below rows * cols (both filled), or
 * the image was recomputed on the host and has no device boards.  ILCC_BAD_ARGUMENT: image or seed outside the last call. */
int32_t ilcc_structure_plan_seed_board(ilcc_structure_plan* plan, uint32_t image, uint32_t seed, int32_t* rows, int32_t* cols,
                                       int32_t* index, int32_t cap, double* energy);

/* the same from the host code (csrc/image_corners_host.cpp; needs no GPU): what ilcc_chessboard_from_corners grows from `seed`
 * before it applies the overlap rule */
int32_t ilcc_chessboard_seed_board(const ilcc_image_corner* corners, int32_t n_corners, int32_t seed, int32_t* rows, int32_t* cols,
                                   int32_t* index, int32_t cap, double* energy);

#ifdef __cplusplus
}
#endif
#endif
