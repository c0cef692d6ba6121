/*
 * ilcc_paired.h -- what a user does with the extrinsic over a WHOLE recording (in libilcc_hip.so): every scan of a bag coloured
 * from the image taken at the same moment, and written as PCD.  With a static rig the merged coloured cloud of a recording is the
 * most telling picture of a good or a bad extrinsic.  Four layers, each usable alone:
 *
 *   header stamps of clouds and images -> the image of every cloud (host)   ilcc_pair_by_stamp
 *   a batch of scans, each with its image -> XYZRGB records (K8b)            ilcc_colourise_plan_*, ilcc_colourise_batch_device
 *   XYZRGB records -> a binary PCD file (host)                               ilcc_save_pcd_xyzrgb
 *   bags -> one coloured cloud per scan                                      ilcc_bag_rgblidar_all_scans; CLI ilcc_rgblidar
 *
 *   reference                                                              here
 *   ---------------------------------------------------------------------  ------------------------------------------------
 *   message_filters::Synchronizer<ApproximateTime> of the two topics        ilcc_pair_by_stamp: the NEAREST header stamp within
 *     (ilcc2/test/rgblidar.cpp:125-130, test/pcd2image.cpp:136-141)           max_dt (deviation 1 below)
 *   cv_bridge::toCvCopy(msg, "bgr8") (rgblidar.cpp:88)                      K11c ilcc_image_to_bgr8_device (ilcc_camera_image.h)
 *   cv::undistort -> rectifyImage, computed and NOT sampled (:47-48,62-64)  K11c with the camera; sample_raw: without (deviation 2)
 *   pcl::fromROSMsg (:87)                                                   K0b  ilcc_pointcloud2_unpack_batch_device (ilcc_sequence.h)
 *   spaceToPlane + image.at<Vec3b>(y, x) per point (:50-74)                 K8b  ilcc_colourise_batch_device, per scan what
 *                                                                                ilcc_colourise_device (ilcc_project.h) writes
 *   pcl::io::savePCDFileBinary / the viewer (:76-78)                        ilcc_save_pcd_xyzrgb
 *
 * Deviation 1, documented: the reference pairs by message_filters::ApproximateTime, whose source is not available to this
 * project.  Here every cloud takes the image whose header stamp is nearest to its own, if that is within max_dt; the rule is
 * written out at ilcc_pair_by_stamp and tests/paired_ref.py restates it by brute force.
 * Deviation 2, documented: the reference undistorts the image into rectifyImage and then samples `image`, the DISTORTED one
 * (rgblidar.cpp:47-66).  spaceToPlane is a pinhole projection without distortion, so the undistorted image is the one its pixels
 * belong to: the chain samples that by default.  sample_raw != 0 restores the reference's behaviour.
 *
 * tests/paired_ref.py is the numpy specification of all four layers.
 */
#ifndef ILCC_PAIRED_H_
#define ILCC_PAIRED_H_

#include "ilcc_camera_image.h"
#include "ilcc_hip.h"
#include "ilcc_project.h"
#include "ilcc_sequence.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- a. pairing (host only; csrc/paired_host.cpp) ----------------------------------------------------------------------------
 * Stamps are header stamps in nanoseconds (sec * 1000000000 + nsec).  Both arrays are in message order and need not be sorted.
 * For cloud i, j is the image with the least |image_ns[j] - cloud_ns[i]|; a tie goes to the lower j.  When |dt| <= max_dt_ns:
 * image_of[i] = j and dt_ns[i] = image - cloud (signed).  Otherwise image_of[i] = -1 and dt_ns[i] is the dt of that nearest image
 * (0 with n_images == 0).  One image may serve several clouds.  A |dt| of 2^63 ns or more counts as beyond every max_dt_ns and is
 * reported as INT64_MAX or INT64_MIN.  A stable sort of the image indices and one binary search per cloud.
 * ILCC_BAD_ARGUMENT: a null pointer with a non-zero count. */
int32_t ilcc_pair_by_stamp(const uint64_t* cloud_ns, uint64_t n_clouds, const uint64_t* image_ns, uint64_t n_images,
                           uint64_t max_dt_ns, int64_t* image_of, int64_t* dt_ns);

/* ---- b. K8b: a batch of scans coloured in one go (csrc/k8b_colourise_batch.hip) ---------------------------------------------
 * d_xyzi + offsets[0 .. n_scans] (host) is the layout K0b writes: scan s is points offsets[s] .. offsets[s + 1].
 * d_images_bgr[k] (host array of device pointers) is a B,G,R image of cam->width x cam->height, rows image_steps[k] bytes apart.
 * image_of_scan[s] is in -1 .. n_images - 1; a scan with -1 yields no records and its points are never read.
 * Output: the 16-byte records of ilcc_colourise_device, scan after scan, input order inside a scan; after
 * ilcc_colourise_plan_finish, out_offsets[s] is the first record of scan s and out_offsets[n_scans] the count of all records.
 * For every scan, d_xyzrgb[out_offsets[s] .. out_offsets[s + 1]) is byte for byte what ilcc_colourise_device writes for that scan
 * alone with that image.  Not a byte behind out_offsets[n_scans] records is written.
 *
 * Three launches however many scans: count per 4096-point chunk (a chunk never straddles two scans), one workgroup that turns
 * the chunk counts into their exclusive prefix and writes the scans' offsets, scatter.  The chunk table and the per-scan table
 * travel through memory the plan owns (page-locked host copy, device copy, one asynchronous upload on hip_stream in front of
 * the launches).  Asynchronous on hip_stream; ilcc_colourise_plan_finish waits for the plan's last call and copies the offsets
 * out.  A plan serves one call at a time: a call first waits for the plan's previous call to have finished on the device.
 * Destroy it only after its last call has finished.  offsets, d_images_bgr, image_steps, image_of_scan and *cam are read
 * before the call returns (the tables built from them are the plan's): the caller may change or free them at once.
 *
 * Refusals -- all on the host, nothing launched or copied, d_xyzrgb untouched: null pointers / more scans or points than the plan
 * holds / decreasing offsets / an image_of_scan outside its range / an image step < 3 * width / width or height <= 0 / more than
 * 2^32 - 2 points (ILCC_BAD_ARGUMENT); cap_points below the points of the paired scans (ILCC_CAPACITY: the device never needs a
 * bounds check on the output).  n_scans == 0 or no paired point: ILCC_OK, zero launches, all offsets 0. */
typedef struct ilcc_colourise_plan ilcc_colourise_plan;
ilcc_colourise_plan* ilcc_colourise_plan_create(uint32_t max_scans, uint64_t max_points);   /* on the current device; NULL on failure (ilcc_last_error(NULL)) */
void ilcc_colourise_plan_destroy(ilcc_colourise_plan* plan);
int32_t ilcc_colourise_batch_device(const void* d_xyzi, const uint64_t* offsets, uint32_t n_scans,
                                    const void* const* d_images_bgr, const uint32_t* image_steps, uint32_t n_images,
                                    const int32_t* image_of_scan, const ilcc_projection* cam, double distance_valid,
                                    void* d_xyzrgb, uint64_t cap_points, ilcc_colourise_plan* plan, void* hip_stream);
/* out_offsets: n_scans + 1 entries of the plan's last accepted call.  ILCC_BAD_ARGUMENT: null pointers or no accepted call. */
int32_t ilcc_colourise_plan_finish(ilcc_colourise_plan* plan, uint64_t* out_offsets);
/* kernel launches of the plan's last accepted call (0 or 3) */
uint32_t ilcc_colourise_plan_launches(const ilcc_colourise_plan* plan);

/* ---- c. PCD writer (host only; csrc/paired_host.cpp) ------------------------------------------------------------------------
 * The binary file PCL 1.8 writes for a pcl::PointCloud<pcl::PointXYZRGB> of n points: the header lines
 *   # .PCD v0.7 - Point Cloud Data file format / VERSION 0.7 / FIELDS x y z rgb / SIZE 4 4 4 4 / TYPE F F F F / COUNT 1 1 1 1 /
 *   WIDTH n / HEIGHT 1 / VIEWPOINT 0 0 0 1 0 0 0 / POINTS n / DATA binary
 * each ending in '\n', then the n 16-byte records as they are.  The header text is restated from memory of PCL's PCDWriter; PCL
 * is not available to this project, tests/paired_ref.py is the specification.  n == 0 writes a valid empty file.
 * ILCC_BAD_ARGUMENT: null filename, or null records with n != 0; ILCC_IO_ERROR when the file cannot be written. */
int32_t ilcc_save_pcd_xyzrgb(const char* filename, const void* xyzrgb, uint64_t n);

/* ---- d. the chain (csrc/paired_api.cpp) ------------------------------------------------------------------------------------- */
typedef struct ilcc_paired_params {
  uint32_t first;               /* first cloud message of the topic that is taken (time order) */
  uint32_t stride;              /* every stride-th from there (0 is read as 1) */
  uint32_t max_scans;           /* at most this many (0: all) */
  int32_t sample_raw;           /* != 0: sample the image as the bag carries it (converted to B,G,R, not undistorted) */
  uint64_t max_dt_ns;           /* a cloud whose nearest image is further away stays unpaired */
  uint64_t staging_bytes;       /* cloud data per batch; 0: 256 MiB */
  uint64_t image_bytes;         /* device bytes (raw + B,G,R) of the distinct images of a batch; 0: 512 MiB */
} ilcc_paired_params;

typedef struct ilcc_pair_record {
  uint32_t message;             /* index of the cloud on its topic */
  uint32_t stamp_sec, stamp_nsec;
  int32_t image_message;        /* index of the image on its topic; -1: unpaired */
  uint32_t image_stamp_sec, image_stamp_nsec;   /* of the NEAREST image, paired or not (0 when the topic's list is empty) */
  int64_t dt_ns;                /* image - cloud, of the nearest image */
  uint64_t n_points, n_coloured;
} ilcc_pair_record;

/* xyzrgb: rec->n_coloured records, valid during the call only.  A non-zero return ends the chain. */
typedef int32_t (*ilcc_pair_sink)(void* user, const ilcc_pair_record* rec, const void* xyzrgb);

/* stride 1, max_dt 50 ms, staging 256 MiB, images 512 MiB, everything else 0 */
void ilcc_default_paired_params(ilcc_paired_params* pp);

/* rgblidar over a recording.  Both topics are opened with ilcc_bag_topic_open (images: the sensor_msgs/Image md5; a topic that
 * carries only sensor_msgs/CompressedImage is refused with ILCC_BAD_ARGUMENT, the text says so).  Every image message's header is
 * read once (ilcc_image_parse_any) for its stamp, size and encoding; an image whose size differs from camera's is
 * ILCC_BAD_ARGUMENT and the text names the message index.  The clouds are selected by first / stride / max_scans as
 * ilcc_sequence_params does and paired with ilcc_pair_by_stamp.
 * A batch is as many consecutive selected scans as keep the clouds' data[] within staging_bytes and the distinct images they
 * need within image_bytes; a single scan or image above its budget is ILCC_CAPACITY.  An image needed by two batches is uploaded
 * twice.  Per batch, on one stream: one H2D copy of the clouds, K0b; per distinct image one H2D copy of data[] and K11c
 * (undistorted with `camera`; sample_raw != 0: camera == NULL); K8b; then finish, one D2H copy of the records, and `sink` once
 * per selected scan in scan order, unpaired scans included (n_coloured = 0).  Two sets of page-locked and device buffers: the
 * host stages the next batch while the device works on this one.
 * T_lidar2cam: row-major 4 x 4, as ilcc_extrinsic_read returns it.  pp == NULL: the defaults.  sink may be NULL (counts only).
 * *n_scans: the selected scans; *n_paired: those with an image.  A non-zero return from sink ends the call with ILCC_IO_ERROR,
 * after what is in flight has been waited for. */
int32_t ilcc_bag_rgblidar_all_scans(int32_t device, const char* image_bag, const char* image_topic, const char* lidar_bag,
                                    const char* lidar_topic, const ilcc_camera_model* camera, const double T_lidar2cam[16],
                                    double distance_valid, const ilcc_paired_params* pp, ilcc_pair_sink sink, void* user,
                                    uint32_t* n_scans, uint32_t* n_paired);

#ifdef __cplusplus
}
#endif
#endif
