/*
 * ilcc_image_corners.h -- the camera half of the calibration input: chessboard corners in an 8-bit
 * grayscale image, as libcbdetect's findCorners + chessboardsFromCorners find them, and the
 * `<camera><i>.txt` file that ilcc_calib_lidar_cam reads.  Implemented in libilcc_hip.so: corner
 * candidates on the GPU (K10, csrc/k10_image_corners.hip), structure recovery and the writer on the
 * host (csrc/image_corners_host.cpp).
 *
 *   reference                                                     here
 *   ------------------------------------------------------------  ----------------------------------------
 *   findCorners.m:31-43      derivatives, angle, weight           k10_gradients (int16 numerators)
 *   findCorners.m:45-49      min / max normalisation              k10_minmax, applied once per pixel
 *   createCorrelationPatch.m, findCorners.m:51-85  likelihood      k10_likelihood (6 classes, fp32)
 *   nonMaximumSuppression.m  n = 3, tau = 0.025, margin 5         k10_nms + host sort into scan order
 *   refineCorners.m (+ edgeOrientations, findModesMeanShift)      k10_refine_score (fp64, one wave each)
 *   scoreCorners.m, cornerCorrelationScore.m  radii 4 / 8 / 12    k10_refine_score
 *   findCorners.m:97-125     edge / tau removal, sign rules, -1   ilcc_image_corners_device (host)
 *   chessboardsFromCorners.m, initChessboard.m, growChessboard.m,
 *   chessboardEnergy.m                                            ilcc_chessboard_from_corners (host)
 *   plotChessboards.m:48-68 (dlmwrite of the X then Y block)      ilcc_save_cam_corners
 *   (a batch of images in one go, every image of a bag fused)     ilcc_image_sequence.h (K10b: the same stage bodies)
 *   (the boards of a batch of corner lists in two launches)        ilcc_image_structure.h (K18: one wavefront per seed corner)
 *
 * Corner positions are 0-based pixels (findCorners.m:124-125); the file adds 1 back, as the
 * reference's dump does.  Not here: multi-board output.  The undistorted image itself
 * (from a bag or a raw frame) comes from ilcc_camera_image.h, the pixels of a .jpg file from ilcc_jpeg.h.
 */
#ifndef ILCC_IMAGE_CORNERS_H_
#define ILCC_IMAGE_CORNERS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* one refined, scored corner: 0-based position, the two edge directions (unit; v1.x + v1.y >= 0,
 * (v1, v2) right-handed) and the correlation score */
typedef struct ilcc_image_corner {
  double u, v;
  double v1[2], v2[2];
  double score;
} ilcc_image_corner;

/* Optional per-stage outputs of ilcc_image_corners_device (any pointer may be NULL). */
typedef struct ilcc_image_corner_stages {
  float* d_likelihood;            /* device, width * height floats (row-major, rows width apart): the corner map */
  int32_t* candidates;            /* host, [capacity][2]: NMS maxima, 1-based (u, v), scan order (u outer) */
  ilcc_image_corner* refined;     /* host, [capacity]: every candidate after refineCorners, 1-based position, */
                                  /*   raw v1 / v2 (zero = no edges), score (0 where not scored) */
  int32_t capacity;               /* entries of candidates / refined */
  int32_t n_candidates;           /* out: number of NMS maxima (may exceed capacity) */
  float ms[4];                    /* out: HIP-event ms of gradients + min/max, likelihood, NMS, refine + score */
} ilcc_image_corner_stages;

/* findCorners(img, tau = 0.01, refine = 1) on an 8-bit grayscale image in device memory (rows
 * `stride` bytes apart).  Writes up to `capacity` corners (host memory) in the reference's order;
 * *n_corners is the full count (ILCC_CAPACITY when it exceeds capacity).  Synchronous on return.
 * Needs width, height >= 34 (2 x 12 + 2 x 5) and stride >= width.  hip_stream: hipStream_t or NULL. */
int32_t ilcc_image_corners_device(const void* d_image, int32_t width, int32_t height, int32_t stride,
                                  ilcc_image_corner* corners, int32_t capacity, int32_t* n_corners,
                                  ilcc_image_corner_stages* stages, void* hip_stream);

/* chessboardsFromCorners on host corners (positions in any consistent frame).  Returns ILCC_OK and
 * the one recovered board with {rows, cols} == {board_w, board_h}, as *rows x *cols corner indices
 * (row-major, into `corners`) in `board_index` (room for board_w * board_h); ILCC_BOARD_NOT_FOUND
 * when there is none, ILCC_AMBIGUOUS when there is more than one.  Host only: needs no GPU. */
int32_t ilcc_chessboard_from_corners(const ilcc_image_corner* corners, int32_t n_corners, int32_t board_w,
                                     int32_t board_h, int32_t* rows, int32_t* cols, int32_t* board_index);

/* Both steps: the board's 0-based (u, v) per matrix entry, row-major, in xy[rows * cols * 2].  Synchronous on return like
 * the first step; the kernels and copies of both entries run on hip_stream. */
int32_t ilcc_find_chessboard_device(const void* d_image, int32_t width, int32_t height, int32_t stride,
                                    int32_t board_w, int32_t board_h, int32_t* rows, int32_t* cols, double* xy,
                                    void* hip_stream);

/* Write a board (0-based xy as above) as plotChessboards dumps it: the X block then the Y block,
 * one line per matrix row, values + 1 as %.5g separated by ' ', lines ended by '\n'. */
int32_t ilcc_save_cam_corners(const char* filename, int32_t rows, int32_t cols, const double* xy);

#ifdef __cplusplus
}
#endif
#endif
