/*
 * ilcc_camera_image.h -- the step BEFORE ilcc_image_corners.h: from a camera bag, or from a raw frame,
 * to the undistorted 8-bit grayscale image in device memory that K10 takes.  Implemented in
 * libilcc_hip.so: the intrinsics reader, the sensor_msgs/Image parser and the bag entries on the host
 * (csrc/camera_image_host.cpp), conversion and undistortion in one gfx950 kernel (K11 for grayscale, K11c for
 * the colour image that ilcc_overlay.h draws LiDAR points on; csrc/k11_camera_image.hip).
 *
 *   reference                                                             here
 *   --------------------------------------------------------------------  ---------------------------
 *   ImageCornersEst::getRectifyParam (src/ImageCornersEst.cpp:15-61)      ilcc_read_camera_yaml
 *     K, d, Camera.width / Camera.height of pointgrey.yaml
 *   rosbag View + first sensor_msgs/Image                                  ilcc_bag_first_message (ilcc_ingest.h)
 *     (test/get_image_corners_bag.cpp:78-84)                                with the Image md5sum
 *   ros::serialization of sensor_msgs/Image (message layout)               ilcc_image_parse, ilcc_image_parse_any
 *   cv_bridge's demosaicing of a raw colour-camera topic (bayer_*8), on    the two K11 entries, per tap
 *     the way to MONO8 or "bgr8"  (cv::cvtColor, COLOR_Bayer*2GRAY / 2BGR)               (csrc/bayer_tap.h)
 *   cv_bridge::toCvCopy(msg, MONO8)  (test/get_image_corners_bag.cpp:26)    ilcc_image_to_mono8_device
 *   undistort_image -> cv::undistort(image, rectify, camK, distort_param,                 (K11, gfx950 kernel)
 *     camK)          (src/ImageCornersEst.cpp:63-66)
 *   cv_bridge::toCvCopy(msg, "bgr8") + cv::undistort of the COLOUR image   ilcc_image_to_bgr8_device
 *     (test/pcd2image.cpp:36,101)                                                        (K11c, gfx950 kernel)
 *   initUndistortRectifyMap's map, as a stage output                      ilcc_undistort_map_device
 *   imwrite of the undistorted image (test/get_image_corners_bag.cpp:110)  ilcc_bag_first_image (host pixels)
 *   ... and the MATLAB step on that image (ilcc_image_corners.h)           ilcc_bag_find_chessboard
 *
 * The arithmetic (OpenCV 3's documented formulas; tests/camera_image_ref.py restates it in numpy):
 *   mono8:  Y = (4899 R + 9617 G + 1868 B + 8192) >> 14; alpha is ignored; mono8 is copied.
 *   map of output pixel (j, i), fp64, unfused, in this order (the four constants once, on the host):
 *     x = j * (1 / fx) + (-cx / fx);  y = i * (1 / fy) + (-cy / fy)
 *     x2 = x x;  y2 = y y;  r2 = x2 + y2;  _2xy = 2 x y;  kr = 1 + ((k3 r2 + k2) r2 + k1) r2
 *     u = fx (x kr + p1 _2xy + p2 (r2 + 2 x2)) + cx;   v = fy (y kr + p1 (r2 + 2 y2) + p2 _2xy) + cy
 *     iu = rint(32 u);  iv = rint(32 v)   (round half to even)
 *   When |32 u| or |32 v| is not below 2^30 (NaN and infinities included) the pixel has no source: both
 *   codes are INT32_MIN and the pixel is 0.
 *   sample: x0 = iu >> 5, y0 = iv >> 5 (arithmetic: floors negative codes), a = iu & 31, b = iv & 31,
 *     weights 32 (32-a)(32-b), 32 a (32-b), 32 (32-a) b, 32 a b; a tap outside the source counts as 0, each
 *     on its own; dst = (sum + 16384) >> 15.  Colour taps are converted to Y first.
 *   bgr8 (K11c): bgr8 is copied, rgb8 swaps channels 0 and 2, bgra8 / rgba8 drop alpha (rgba8 also swaps), mono8 is
 *     replicated into the three channels; with a camera, the same codes and the same four weights blend each of
 *     B, G, R on its own (the conversion permutes or replicates channels, so it commutes with the blend).
 *   Bayer sources (bayer_rggb8, bayer_bggr8, bayer_gbrg8, bayer_grbg8; one byte per pixel, the name gives the colours
 *   of pixels (0,0) (1,0) of row 0 and (0,1) (1,1) of row 1, period 2 on both axes, odd sizes allowed) are demosaiced as
 *   OpenCV 3's scalar Bayer2RGB_ / Bayer2Gray_ do it (imgproc/src/demosaicing.cpp), which cv_bridge reaches with
 *   bayer_rggb8 -> COLOR_BayerBG2*, bggr8 -> BayerRG, gbrg8 -> BayerGR, grbg8 -> BayerGB.  S(x, y): the raw byte.
 *     interior (1 <= x <= w-2, 1 <= y <= h-2), integer sums:
 *       at an R or B site: own colour S(x,y); G = (S(x-1,y) + S(x+1,y) + S(x,y-1) + S(x,y+1) + 2) >> 2;
 *         the opposite colour (S(x-1,y-1) + S(x+1,y-1) + S(x-1,y+1) + S(x+1,y+1) + 2) >> 2
 *       at a G site: G = S(x,y); the colour of this row's non-green sites (S(x-1,y) + S(x+1,y) + 1) >> 1; the other
 *         colour (S(x,y-1) + S(x,y+1) + 1) >> 1
 *       gray, from the raw sums (NOT the gray of that B,G,R: one rounding, not two), cR = 4899, cG = 9617, cB = 1868:
 *         R / B site: Y = (4 c_own S(x,y) + cG (the 4 cross neighbours) + c_opp (the 4 diagonals) + 32768) >> 16
 *         G site:     Y = (2 cG S(x,y) + c_h (S(x-1,y) + S(x+1,y)) + c_v (S(x,y-1) + S(x,y+1)) + 16384) >> 15,
 *                     c_h / c_v: the coefficient of the row's / the column's non-green colour
 *     border: D(x, y) = I(clamp(x, 1, w-2), clamp(y, 1, h-2)), I the interior rule, colour and gray (OpenCV copies
 *       column 1 into column 0 and column w-2 into column w-1, then row 1 into row 0 and row h-2 into row h-1)
 *     with a camera the map, the codes, the weights and the rounding are the ones above: a tap inside the source is
 *       D(x, y) (gray for mono8; B, G, R each blended on its own for bgr8), a tap outside counts as 0.
 *     OpenCV's vectorised gray path works in 16-bit mulhi arithmetic and may differ from its own scalar path by a grey
 *     level; the scalar path is what is specified here.  The colour path is exact in both.
 *     Deviation: a Bayer image with width < 3 or height < 3 is refused (OpenCV returns zeros there).
 *   Deviation from OpenCV: it accumulates x along a row and works in stripes; here every pixel is
 *   evaluated directly (order 1e-13 px: moves a 1/32-pixel code only at an exact tie).
 *
 * A topic that carries no sensor_msgs/Image but sensor_msgs/CompressedImage (JPEG) is read by the two bag entries
 * all the same: K13 (ilcc_jpeg.h) decodes its first message into the frame K11 then takes.
 *
 * Not here: 16-bit encodings (mono16, bayer_*16); the rational (k4..k6), thin-prism and tilt terms of the distortion
 * model; the stereo rectification of undistort_stereo_image; structure recovery stays on the host
 * (ilcc_image_corners.h).
 */
#ifndef ILCC_CAMERA_IMAGE_H_
#define ILCC_CAMERA_IMAGE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* pinhole intrinsics (zero skew), OpenCV's distortion coefficients in its order, and the image size */
typedef struct ilcc_camera_model {
  double fx, fy, cx, cy;
  double d[5];                  /* k1, k2, p1, p2, k3 */
  int32_t width, height;
} ilcc_camera_model;

enum ilcc_image_encoding {
  ILCC_ENCODING_MONO8 = 0,
  ILCC_ENCODING_BGR8 = 1,
  ILCC_ENCODING_RGB8 = 2,
  ILCC_ENCODING_BGRA8 = 3,
  ILCC_ENCODING_RGBA8 = 4,
  /* 5 .. 15: not used, refused.  Raw colour-camera frames, one byte per pixel; taken by ilcc_image_parse_any, the two
   * K11 entries and the bag entries, not by ilcc_image_parse nor by ilcc_jpeg_write.h */
  ILCC_ENCODING_BAYER_RGGB8 = 16,
  ILCC_ENCODING_BAYER_BGGR8 = 17,
  ILCC_ENCODING_BAYER_GBRG8 = 18,
  ILCC_ENCODING_BAYER_GRBG8 = 19
};

typedef struct ilcc_image_layout {
  uint32_t height, width;
  uint32_t step;                /* bytes from one row to the next */
  uint32_t encoding;            /* ilcc_image_encoding */
  uint32_t is_bigendian;
  uint32_t stamp_sec, stamp_nsec, seq;
  uint64_t data_offset;         /* of data[] inside the serialized message */
  uint64_t data_bytes;
  char frame_id[64];
} ilcc_image_layout;

/* K (3 x 3, dt: d), d (4 or 5 entries, a column or a row; a missing k3 is 0) and Camera.width /
 * Camera.height of an OpenCV-FileStorage YAML.  ILCC_IO_ERROR: unreadable file; ILCC_BAD_ARGUMENT: a
 * key is missing or malformed, K has skew or a last row other than (0, 0, 1).  Host only. */
int32_t ilcc_read_camera_yaml(const char* path, ilcc_camera_model* out);

/* layout of a serialized sensor_msgs/Image (md5sum 060021388200f6f0f447d0fcd9c64743).  Refused with
 * ILCC_BAD_ARGUMENT: a truncated message or a length field that runs past it, an empty image, an
 * encoding other than mono8 .. rgba8 (the last-error text names it; the Bayer names too: layout.encoding is 0 .. 4), step < width * bytes per
 * pixel, data_bytes < step * height.  Allocates nothing.  Host only. */
int32_t ilcc_image_parse(const uint8_t* msg, uint64_t msg_bytes, ilcc_image_layout* out);

/* ilcc_image_parse plus bayer_rggb8, bayer_bggr8, bayer_gbrg8 and bayer_grbg8 (layout.encoding 16 .. 19, step >= width);
 * a Bayer image narrower or lower than 3 pixels is refused.  What the bag entries read a topic's frame with. */
int32_t ilcc_image_parse_any(const uint8_t* msg, uint64_t msg_bytes, ilcc_image_layout* out);

/* K11: pixels of `encoding` in device memory (rows src_step bytes apart) -> 8-bit grayscale in device
 * memory (rows dst_stride bytes apart): cv::undistort(mono8(src), K, d, K) with a camera, mono8(src)
 * with camera == NULL.  On hip_stream (a hipStream_t, NULL = default stream); asynchronous; *camera is read
 * before the call returns (in this entry and in the two below).  Checked on
 * the host before any launch (ILCC_BAD_ARGUMENT): null pointers, width / height outside 1 .. 65536,
 * strides shorter than a row, an unknown encoding, a Bayer image below 3 x 3, a camera of another size or with fx or fy not
 * finite and non-zero, source and destination ranges that overlap (the kernel gathers). */
int32_t ilcc_image_to_mono8_device(const void* d_src, int32_t width, int32_t height, int32_t src_step, int32_t encoding,
                                   const ilcc_camera_model* camera, void* d_dst, int32_t dst_stride, void* hip_stream);

/* K11c: cv_bridge::toCvCopy(msg, "bgr8") followed by cv::undistort(image, K, d, K) (pcd2image.cpp:36,101):
 * pixels of `encoding` -> 3 bytes B,G,R per pixel, rows dst_stride bytes apart.  camera == NULL: conversion only.
 * The checks of the mono8 entry with dst_stride >= 3 * width; not a byte outside
 * [row * dst_stride, row * dst_stride + 3 * width) is written.  Asynchronous on hip_stream. */
int32_t ilcc_image_to_bgr8_device(const void* d_src, int32_t width, int32_t height, int32_t src_step, int32_t encoding,
                                  const ilcc_camera_model* camera, void* d_dst, int32_t dst_stride, void* hip_stream);

/* Stage output of K11: the 1/32-pixel source coordinates of every output pixel, camera->width x
 * camera->height int32 each (device memory, row-major, packed).  Asynchronous on hip_stream. */
int32_t ilcc_undistort_map_device(const ilcc_camera_model* camera, int32_t* d_iu, int32_t* d_iv, void* hip_stream);

/* bag -> host pixels: the first sensor_msgs/Image on `topic` (the first CompressedImage when it has none), converted (and undistorted when camera is
 * not NULL) on device `device`, width x height bytes, packed.  *width / *height are the image's even when
 * cap_bytes is too small (ILCC_CAPACITY). */
int32_t ilcc_bag_first_image(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera,
                             uint8_t* mono8_out, uint64_t cap_bytes, int32_t* width, int32_t* height);

/* The same chain with the image kept on the device and handed to ilcc_find_chessboard_device: rows, cols
 * and xy as there (what ilcc_save_cam_corners takes). */
int32_t ilcc_bag_find_chessboard(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera,
                                 int32_t board_w, int32_t board_h, int32_t* rows, int32_t* cols, double* xy);

#ifdef __cplusplus
}
#endif
#endif
