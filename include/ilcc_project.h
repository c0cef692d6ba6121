/*
 * ilcc_project.h -- the step AFTER calibration: per-point LiDAR -> image
 * projection with the calibrated extrinsic, and the drawing of the projected points into the image.
 * Implemented in libilcc_hip.so (K8 and K12, gfx950 kernels).
 *
 *   reference                                                            here
 *   -------------------------------------------------------------------  -------------------------------
 *   ImageCornersEst::spaceToPlane   (ilcc2/src/ImageCornersEst.cpp:135-155)  both entries, per point
 *   ImageCornersEst::HSVtoRGB       (:373-428)                               ilcc_project_intensity_device
 *   pcd2image processData loop      (ilcc2/test/pcd2image.cpp:40-82)         ilcc_project_intensity_device
 *   rgblidar  processData loop      (ilcc2/test/rgblidar.cpp:45-78)          ilcc_colourise_device
 *   cv::circle(image, Point(x, y), 0.6, Scalar(r, g, b), 2) per hit (pcd2image.cpp:75)  ilcc_draw_hits_device (K12)
 *
 * The stamp of that cv::circle: the radius is an int, so 0.6 becomes 0; with thickness 2 OpenCV 3 goes EllipseEx ->
 * PolyLine -> ThickLine on a zero-length segment, which draws a filled Circle of radius (2 * 2^15 + 2^15) >> 16 = 1,
 * and its midpoint loop fills row y: x-1 .. x+1 and rows y-1, y+1: x only -- the centre and its four neighbours, 5 pixels.
 * (Restated from OpenCV 3's source; OpenCV is not available to the tests, tests/overlay_ref.py is the specification.)
 * Colour order: Scalar(r, g, b) on a bgr8 image puts r into byte 0, so the reference's window shows red and blue swapped.
 * K12 writes (r, g, b) into bytes 0, 1, 2 all the same; ilcc_save_ppm_bgr (ilcc_overlay.h) turns B,G,R into R,G,B, so its
 * file shows what the reference's window showed.
 *
 * Not here: cv::undistort of the image (ilcc_image_to_bgr8_device, ilcc_camera_image.h), imshow (display), the ROS
 * subscribers (ilcc_overlay.h chains bag -> picture); anti-aliased drawing.  The projection
 * entries keep the reference's quirks: spaceToPlane accepts P_c.z == 0 (division by zero -> inf/NaN
 * fails the image test), pixel = (int) truncation, rgblidar samples the image it was GIVEN (the
 * reference passes the distorted one, rgblidar.cpp:62-64), pcd2image's fixed colour range 0..60.
 */
#ifndef ILCC_PROJECT_H_
#define ILCC_PROJECT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ilcc_projection {
  double R[9];            /* m_R, row-major: lidar -> camera rotation (ImageCornersEst::setRt) */
  double t[3];            /* m_t */
  double fx, cx, fy, cy;  /* m_fx ... from camK */
  int32_t width, height;  /* m_image_size */
} ilcc_projection;

/* one projected point: integer pixel, colour, index of the source point */
typedef struct ilcc_pixel_hit {
  int32_t x, y;
  uint8_t r, g, b, pad;
  uint32_t index;
} ilcc_pixel_hit;

/* pcd2image: hits (input order) of the points that pass spaceToPlane, coloured by
 * HSVtoRGB((intensity - inten_low) / (inten_high - inten_low) * 255, 100, 100); the reference fixes
 * inten_low = 0, inten_high = 60.  d_hits has room for n_points records.  Synchronous on return
 * (*n_hits is a host value).  hip_stream: hipStream_t or NULL. */
int32_t ilcc_project_intensity_device(const void* d_xyzi, uint32_t n_points, const ilcc_projection* cam,
                                      double distance_valid, double inten_low, double inten_high, void* d_hits,
                                      uint32_t* n_hits, void* hip_stream);

/* rgblidar: XYZRGB cloud (input order) of the points that pass spaceToPlane, colour = the BGR pixel
 * at (int)u, (int)v of d_image_bgr (rows image_step bytes apart).  Output records are 16 bytes:
 * float x, y, z and PCL's packed rgb (uint32 r << 16 | g << 8 | b, stored in the 4th float's bits).  Synchronous on
 * return like the entry above (*n_out is a host value); both read *cam before they launch. */
int32_t ilcc_colourise_device(const void* d_xyzi, uint32_t n_points, const ilcc_projection* cam,
                              double distance_valid, const void* d_image_bgr, uint32_t image_step, void* d_xyzrgb,
                              uint32_t* n_out, void* hip_stream);

/* K12.  pcd2image.cpp:75: cv::circle(image, Point(x, y), 0.6, Scalar(r, g, b), 2) for every hit, in the order of d_hits.
 * d_image_bgr (rows stride bytes apart) is drawn into in place: the result is the image a sequential loop leaves -- for
 * hit k = 0 .. n_hits-1 and every stamp offset (dx, dy), bytes 0, 1, 2 of pixel (x+dx, y+dy) become (r, g, b) when that
 * pixel is inside the image; a later hit overwrites an earlier one, each stamp pixel is clipped on its own, and x, y may be
 * any int32.  d_scratch: ilcc_draw_hits_scratch_bytes(width, height) bytes of device memory, contents irrelevant on
 * entry.  stamp_xy == NULL: the reference's stamp; else n_stamp (1..64) pairs (dx, dy) of int8 in HOST memory, read
 * before the call returns.  d_scratch belongs to the call until its launches have run: two calls in flight need two.
 * Asynchronous on hip_stream; the result does not depend on thread order.  ILCC_BAD_ARGUMENT before any launch: null
 * pointers, width / height outside 1..65536, stride < 3 * width, n_stamp outside 1..64 with a stamp given,
 * n_hits > 2^32 - 2, d_hits or d_scratch not 4-byte aligned.  n_hits == 0: ILCC_OK, nothing is touched. */
uint64_t ilcc_draw_hits_scratch_bytes(int32_t width, int32_t height);
int32_t ilcc_draw_hits_device(void* d_image_bgr, int32_t width, int32_t height, int32_t stride, const void* d_hits,
                              uint32_t n_hits, const int8_t* stamp_xy, int32_t n_stamp, void* d_scratch, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
