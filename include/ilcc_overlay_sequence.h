/*
 * ilcc_overlay_sequence.h -- pcd2image over a WHOLE recording (in libilcc_hip.so): every scan of a bag drawn on the image taken
 * at the same moment.  The reference's node shows a moving overlay, and the user watches it for dots that slide off the scene's
 * edges; ilcc_overlay.h draws one picture, from the first message of each topic.  The layers, each usable alone:
 *
 *   header stamps of clouds and images -> the image of every cloud (host)     ilcc_pair_by_stamp (ilcc_paired.h)
 *   PointCloud2 messages of a batch -> XYZI (K0b)                             ilcc_pointcloud2_unpack_batch_device (ilcc_sequence.h)
 *   a batch of scans, each with its image -> one drawn canvas per scan (K12b) ilcc_overlay_plan_*, ilcc_overlay_batch_device
 *   a packed array of B,G,R pictures -> JPEG scans (K14b, K17)                ilcc_jpeg_fdct_batch_device with ILCC_ENCODING_BGR8,
 *                                                                               ilcc_jpeg_huffman_encode_batch_device
 *                                                                               (ilcc_jpeg_write_sequence.h)
 *   the device bytes a paired scan takes in the chain (host)                  ilcc_overlay_sequence_bytes
 *   bags -> one .jpg (and picture) per scan                                   ilcc_bag_pcd2image_all_pairs; CLI ilcc_pcd2image --all-pairs
 *
 *   reference                                                              here
 *   ---------------------------------------------------------------------  ------------------------------------------------
 *   message_filters::Synchronizer<ApproximateTime> of the two topics        ilcc_pair_by_stamp: the NEAREST header stamp within
 *     (ilcc2/test/pcd2image.cpp:136-141)                                      max_dt (ilcc_paired.h, deviation 1 there)
 *   cv_bridge::toCvCopy(msg, "bgr8") + cv::undistort (:36,101)              K11c ilcc_image_to_bgr8_device (ilcc_camera_image.h)
 *   pcl::fromROSMsg (:100)                                                  K0b  ilcc_pointcloud2_unpack_batch_device
 *   spaceToPlane + HSVtoRGB per point (:53-73) and                          K12b ilcc_overlay_batch_device: per scan what
 *     cv::circle(rectifyImage, Point(x, y), 0.6, Scalar(r, g, b), 2) (:75)       ilcc_project_intensity_device followed by
 *     for every point of the cloud, on a copy of the image                       ilcc_draw_hits_device (ilcc_project.h) leave
 *   cv::imshow (:87)                                                        K14b + K17: <prefix><cloud message>.jpg, what
 *                                                                                ilcc_jpeg_write_file writes for the picture
 *
 * The quirks of the single-scan entries are kept: Scalar(r, g, b) on a bgr8 image puts r into byte 0, the colour range is the
 * caller's (the reference fixes 0 .. 60), the stamp is the five pixels of ilcc_project.h unless the caller gives another.
 *
 * Not here: sensor_msgs/CompressedImage topics in the chain; a batched K11c; anti-aliased drawing; show_calib_result's circles and
 * text; video containers.  tests/overlay_sequence_ref.py is the numpy specification of K12b and of the chain.
 */
#ifndef ILCC_OVERLAY_SEQUENCE_H_
#define ILCC_OVERLAY_SEQUENCE_H_

#include <stdint.h>

#include "ilcc_camera_image.h"
#include "ilcc_hip.h"
#include "ilcc_project.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- K12b: a batch of scans projected, coloured and drawn in one go (csrc/k12b_overlay_batch.hip) -------------------------------
 * Inputs as K8b takes them (ilcc_paired.h): d_xyzi + offsets[0 .. n_scans] (host) is the layout K0b writes, scan s is points
 * offsets[s] .. offsets[s + 1]; d_images_bgr[k] (host array of device pointers) is a B,G,R image of cam->width x cam->height,
 * rows image_steps[k] bytes apart; image_of_scan[s] is in -1 .. n_images - 1.  stamp_xy / n_stamp as ilcc_draw_hits_device takes
 * them: NULL for the reference's five pixels, else n_stamp (1 .. 64) pairs (dx, dy) of int8 in host memory.
 *
 * Output: one canvas per scan at d_canvas + s * canvas_pitch, packed B,G,R rows canvas_stride bytes apart -- the array
 * ilcc_jpeg_fdct_batch_device reads with image_pitch = canvas_pitch and src_stride = canvas_stride -- and n_drawn[s], handed out
 * by ilcc_overlay_plan_finish.
 *
 * CONTRACT.  For every paired scan (image_of_scan[s] >= 0) the first 3 * width bytes of every canvas row equal, byte for byte,
 * what these three steps leave for that scan alone: a copy of image image_of_scan[s] into the canvas;
 * ilcc_project_intensity_device on the scan's points; ilcc_draw_hits_device with those hits on the canvas.  n_drawn[s] is that
 * call's *n_hits.  The bytes between 3 * width and canvas_stride, and between a canvas's last row and canvas_pitch, are not
 * written.  An unpaired scan's canvas is not touched, its points are never read, n_drawn[s] = 0.  An empty paired scan yields a
 * plain copy of its image.  Two scans that share an image get canvases of their own: neither shows the other's dots.  Nothing is
 * written behind the last row of canvas n_scans - 1.  The canvases must not overlap the images or each other.
 *
 * Launches, however many scans: THREE -- k12b_prepare (copies each paired scan's image into its canvas and zeroes its owner
 * words), k12b_mark and k12b_resolve (one workgroup per chunk of at most 4096 points, a chunk never straddles two scans; the
 * chunk table is K8b's).  ONE, the prepare alone, when every paired scan is empty: the canvases still receive their images.
 * ZERO when there are no scans or none is paired.  The tables travel through memory the plan owns (page-locked host copy, device
 * copy, one asynchronous upload in front of the launches); the counts come back by one asynchronous copy behind them.
 *
 * d_scratch: ilcc_overlay_batch_scratch_bytes(width, height, n_scans) bytes, 16-byte aligned, contents irrelevant on entry: an
 * owner word per pixel and scan, scan s's plane at s * (4 * width * height rounded up to 16).  It belongs to the call until its
 * launches have run.
 *
 * Asynchronous on job->hip_stream, no allocation, no host wait for the work of THIS call.  A plan serves one call at a time: a
 * call first waits for the plan's previous call to have finished on the device.  Destroy a plan only after its last call has
 * finished.  *job and everything it points to in host memory (offsets, d_images_bgr, image_steps, image_of_scan, *cam, stamp_xy)
 * are read before the call returns.
 *
 * Refusals -- all on the host, nothing launched or copied, canvases and scratch untouched (ILCC_BAD_ARGUMENT): a null job, plan
 * or cam, null arrays with a non-zero count / more scans or points than the plan holds / decreasing offsets / an image_of_scan
 * outside its range / a null image or an image step < 3 * width of a paired scan / more than 2^32 - 2 points (all as
 * ilcc_colourise_batch_device); width or height outside 1 .. 65536 / n_stamp outside 1 .. 64 with a stamp given (as
 * ilcc_draw_hits_device); canvas_stride < 3 * width; canvas_pitch < canvas_stride * (height - 1) + 3 * width; with a paired
 * scan: null d_canvas or d_scratch, scratch_bytes below ilcc_overlay_batch_scratch_bytes, d_scratch not 16-byte aligned; null
 * d_xyzi with a paired point. */
typedef struct ilcc_overlay_plan ilcc_overlay_plan;

typedef struct ilcc_overlay_batch_job {
  const void* d_xyzi;
  const uint64_t* offsets;              /* n_scans + 1, host */
  const void* const* d_images_bgr;      /* n_images device pointers, host */
  const uint32_t* image_steps;          /* n_images, host */
  const int32_t* image_of_scan;         /* n_scans, host */
  const ilcc_projection* cam;
  const int8_t* stamp_xy;               /* NULL: the reference's stamp */
  void* d_canvas;
  void* d_scratch;
  ilcc_overlay_plan* plan;
  void* hip_stream;
  uint64_t canvas_pitch;                /* bytes from one scan's canvas to the next */
  uint64_t scratch_bytes;
  double distance_valid;
  double inten_low, inten_high;         /* the reference fixes 0 and 60 */
  uint32_t n_scans, n_images;
  int32_t canvas_stride;                /* bytes from one canvas row to the next */
  int32_t n_stamp;
} ilcc_overlay_batch_job;               /* 144 bytes */

/* on the current device; max_scans 1 .. 65535, max_points 1 .. 2^32 - 2; NULL on failure (ilcc_last_error(NULL)) */
ilcc_overlay_plan* ilcc_overlay_plan_create(uint32_t max_scans, uint64_t max_points);
void ilcc_overlay_plan_destroy(ilcc_overlay_plan* plan);
/* n_scans * (4 * width * height rounded up to 16); 0 for a size the entry refuses */
uint64_t ilcc_overlay_batch_scratch_bytes(int32_t width, int32_t height, uint32_t n_scans);
int32_t ilcc_overlay_batch_device(const ilcc_overlay_batch_job* job);
/* waits for the plan's last accepted call; n_drawn_out: its n_scans entries.  ILCC_BAD_ARGUMENT: null pointers or no accepted call. */
int32_t ilcc_overlay_plan_finish(ilcc_overlay_plan* plan, uint32_t* n_drawn_out);
/* kernel launches of the plan's last accepted call (0, 1 or 3) */
uint32_t ilcc_overlay_plan_launches(const ilcc_overlay_plan* plan);

/* ---- the device bytes of one paired scan (host only; csrc/overlay_sequence_host.cpp) ------------------------------------------
 * What one PAIRED scan takes on the device in the chain below, beside its cloud and its image (which have budgets of their own),
 * with up(x) = x rounded up to 256 and I = ilcc_jpeg_write_info(width, height, 3, 2, 2, ...), the 4:2:0 file ilcc_jpeg_write_file
 * writes:
 *   up(3 * width * height)             the canvas, packed rows
 *   + up(4 * width * height)           K12b's owner words
 *   + up(2 * I.coef_count)             K14b's coefficients
 *   + up(ilcc_jpeg_fdct_scratch_bytes(I))   K14b's padded Y, Cb, Cr planes
 *   + up(out) + 256                    K17's output, out = out_bytes_per_image (0: width * height) rounded up to 16; the image's row
 *   + ilcc_jpeg_huffman_encode_scratch_bytes(I, 1, out)   K17's scratch for one image; a batch's is never more than its images' sum
 * -- the last four are what ilcc_jpeg_write_sequence_bytes counts, for a 3-component image.  The chain cuts its batches with it.
 * 0 for a size the writer refuses (outside 1 .. 65535) or that K17 refuses. */
uint64_t ilcc_overlay_sequence_bytes(int32_t width, int32_t height, uint64_t out_bytes_per_image);

/* ---- the chain (csrc/overlay_sequence_api.cpp) ---------------------------------------------------------------------------------- */
typedef struct ilcc_overlay_sequence_params {
  uint32_t first;               /* first cloud message of the topic that is taken (time order) */
  uint32_t stride;              /* every stride-th from there (0 is read as 1) */
  uint32_t max_scans;           /* at most this many (0: all) */
  uint32_t route;               /* 0: K17.  1: the host encoder per image, from its coefficients.  Anything else: ILCC_BAD_ARGUMENT */
  uint32_t keep_pixels;         /* != 0: the sink also receives the drawn picture */
  uint32_t reserved;
  uint64_t max_dt_ns;           /* a cloud whose nearest image is further away stays unpaired */
  uint64_t staging_bytes;       /* cloud data per batch; 0: 256 MiB */
  uint64_t image_bytes;         /* device bytes (raw + B,G,R) of the distinct images of a batch; 0: 512 MiB */
  uint64_t device_bytes;        /* ilcc_overlay_sequence_bytes per paired scan of a batch; 0: 1 GiB */
  uint64_t out_bytes_per_image; /* room in K17's output per picture of a batch; 0: width * height */
} ilcc_overlay_sequence_params;   /* 64 bytes */

typedef struct ilcc_overlay_record {
  uint32_t message;             /* index of the cloud on its topic */
  uint32_t stamp_sec, stamp_nsec;
  int32_t image_message;        /* index of the image on its topic; -1: unpaired */
  uint32_t image_stamp_sec, image_stamp_nsec;   /* of the NEAREST image, paired or not (0 when the topic's list is empty) */
  int64_t dt_ns;                /* image - cloud, of the nearest image */
  uint64_t n_points;
  uint32_t n_drawn;
  uint32_t route;               /* the route THIS picture took: 0 K17, 1 the host encoder (asked for, or the capacity fallback) */
  uint64_t file_bytes;          /* 0 for an unpaired scan */
} ilcc_overlay_record;          /* 56 bytes */

/* jpeg: the file's file_bytes bytes; bgr: the picture, packed B,G,R rows of 3 * width bytes, with keep_pixels, else NULL.  Both NULL
 * for an unpaired scan.  Valid during the call only.  A non-zero return ends the chain. */
typedef int32_t (*ilcc_overlay_sink)(void* user, const ilcc_overlay_record* rec, const uint8_t* jpeg, uint64_t jpeg_bytes, const uint8_t* bgr);

/* stride 1, max_dt 50 ms, staging 256 MiB, images 512 MiB, device 1 GiB, everything else 0 */
void ilcc_default_overlay_sequence_params(ilcc_overlay_sequence_params* sp);

/* pcd2image over a recording.  Scan selection (first / stride / max_scans), pairing (max_dt_ns), the image rules and the staging
 * and image budgets are ilcc_bag_rgblidar_all_scans's (ilcc_paired.h): a topic that carries only sensor_msgs/CompressedImage is
 * refused with ILCC_BAD_ARGUMENT and the text says so; an image whose size differs from camera's is ILCC_BAD_ARGUMENT and the
 * text names the message index.  A batch is as many consecutive selected scans as keep the clouds' data[] within staging_bytes
 * and the distinct images they need within image_bytes -- the same cut as ilcc_bag_rgblidar_all_scans makes -- and the paired
 * scans' ilcc_overlay_sequence_bytes within device_bytes; all cut before anything is allocated; a single scan or image above a
 * budget is ILCC_CAPACITY.  An unpaired scan is counted in the cut like any other, but it is never staged or uploaded: it becomes
 * a record.  Per batch, on one stream: one H2D copy of the paired clouds, K0b; per distinct image one
 * H2D copy of data[] and K11c (undistorted with `camera`); K12b with inten 0 .. 60 and the reference's stamp; K14b (BGR8, 4:2:0,
 * the Annex-K tables at `quality`, no restart interval: what ilcc_jpeg_write_file writes); K17; device to host the rows, then ONE
 * copy of the scans that were produced (and of the canvases with keep_pixels).  A picture K17 flags ILCC_JPEG_ENCODE_CAPACITY is
 * finished by the host encoder from its coefficients; with route 1 every picture goes that way.  Two sets of page-locked and
 * device buffers: the host reads and stages batch k + 1 while the device works on k, and encodes, assembles and sinks batch k
 * while the device works on k + 1.  `sink` is called once per selected scan, in scan order; it may be NULL (counts only).
 * CONTRACT: for every paired scan, jpeg equals, byte for byte, ilcc_jpeg_write_file's file for bgr (BGR8, the same quality), and
 * bgr equals K11c -> K0 -> K8 -> K12 on that cloud and that image alone (ilcc_bag_pcd2image's picture); neither depends on how the
 * batches were cut or on `route`.
 * T_lidar2cam: row-major 4 x 4.  sp == NULL: the defaults.  *n_scans: the selected scans; *n_paired: those with an image.  A
 * non-zero return from sink ends the call with ILCC_IO_ERROR, after what is in flight has been waited for. */
int32_t ilcc_bag_pcd2image_all_pairs(int32_t device, const char* image_bag, const char* image_topic, const char* lidar_bag,
                                     const char* lidar_topic, const ilcc_camera_model* camera, const double T_lidar2cam[16],
                                     double distance_valid, int32_t quality, const ilcc_overlay_sequence_params* sp,
                                     ilcc_overlay_sink sink, void* user, uint32_t* n_scans, uint32_t* n_paired);

#ifdef __cplusplus
}
#endif
#endif
