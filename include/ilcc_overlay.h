/*
 * ilcc_overlay.h -- what a user does with the extrinsic once it is calibrated: the reference's pcd2image node
 * (ilcc2/test/pcd2image.cpp:33-89) without ROS or OpenCV.  It undistorts the COLOUR image and draws every LiDAR
 * point that projects into it as a small dot coloured by intensity; whether the dots sit on the scene's edges is
 * how the user sees that the calibration is right.  Implemented in libilcc_hip.so (csrc/overlay_host.cpp) over the
 * stages of the other headers:
 *
 *   reference                                                             here
 *   --------------------------------------------------------------------  ---------------------------------
 *   message_filters::Synchronizer<ApproximateTime> of the two topics       the FIRST message of each topic
 *     (test/pcd2image.cpp:136-141)                                           (ilcc_bag_first_message, ilcc_ingest.h)
 *   cv_bridge::toCvCopy(msg, "bgr8") + cv::undistort (:36,101)             K11c ilcc_image_to_bgr8_device (ilcc_camera_image.h)
 *   pcl::fromROSMsg (:100)                                                 K0   ilcc_pointcloud2_unpack_device (ilcc_ingest.h)
 *   spaceToPlane + HSVtoRGB per point, inten 0 .. 60 (:53-73)              K8   ilcc_project_intensity_device (ilcc_project.h)
 *   cv::circle(rectifyImage, Point(x, y), 0.6, Scalar(r, g, b), 2) (:75)   K12  ilcc_draw_hits_device (ilcc_project.h)
 *   cv::imshow (:87)                                                       ilcc_save_ppm_bgr; CLI ilcc_pcd2image
 *
 * Deviation, documented: the reference pairs image and cloud by ApproximateTime; this entry takes the first message of
 * each topic, like every other bag entry of this library.  For every time-paired scan and image of a recording, drawn in one
 * batch, see ilcc_overlay_sequence.h (K12b).  Quirk, kept: Scalar(r, g, b) on a bgr8 image puts r into
 * byte 0, so the reference's window shows red and blue swapped; ilcc_save_ppm_bgr writes B,G,R as R,G,B, so the file
 * shows what that window showed.
 *
 * Not here: show_calib_result's radius-1 circles and putText; anti-aliased drawing; display.  (JPEG output of the picture:
 * ilcc_jpeg_write.h; CLI ilcc_pcd2image --jpg-out.  rgblidar over every time-paired scan and image of a recording: ilcc_paired.h.)
 */
#ifndef ILCC_OVERLAY_H_
#define ILCC_OVERLAY_H_

#include <stdint.h>

#include "ilcc_camera_image.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pcd2image without ROS: first sensor_msgs/Image on image_topic of image_bag, first PointCloud2 on lidar_topic of
 * lidar_bag (may be the same file), K11c, K0, K8 (inten 0..60 as the reference fixes them), K12, on device `device`
 * with one device allocation for the whole call.  T_lidar2cam: row-major 4 x 4, as ilcc_extrinsic_read returns it.
 * bgr_out: 3 * width * height bytes, packed.  *width / *height are set even on ILCC_CAPACITY.  *n_drawn: the hits
 * K8 found (points that project into the image within distance_valid). */
int32_t ilcc_bag_pcd2image(int32_t device, const char* image_bag, const char* image_topic, const char* lidar_bag,
                           const char* lidar_topic, const ilcc_camera_model* camera, const double T_lidar2cam[16],
                           double distance_valid, uint8_t* bgr_out, uint64_t cap_bytes, int32_t* width, int32_t* height,
                           uint32_t* n_drawn);

/* binary PPM (P6, maxval 255) of a packed B,G,R image, written as R,G,B.  ILCC_IO_ERROR when the file cannot be written.
 * Host only. */
int32_t ilcc_save_ppm_bgr(const char* filename, const uint8_t* bgr, int32_t width, int32_t height);

#ifdef __cplusplus
}
#endif
#endif
