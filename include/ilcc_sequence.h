/*
 * ilcc_sequence.h -- corners from EVERY scan of a recording (in libilcc_hip.so).
 *
 * The reference's get_lidar_corners stops after the first PointCloud2 of a bag (ilcc2/test/get_lidar_corners.cpp:136-164), and so
 * do the entries of ilcc_ingest.h.  A calibration bag holds a board that stands still for seconds: tens to hundreds of scans.
 * The entries here read all of them, unpack a batch of messages in one go (K0b), run the ordinary batch pipeline on them and fuse
 * the per-scan corners into one set.  Four layers, each usable alone:
 *
 *   every message of a topic, in time order (host)             ilcc_bag_topic_*
 *   a batch of PointCloud2 data[] -> concatenated float4 (K0b)  ilcc_unpack_plan_*, ilcc_pointcloud2_unpack_batch_device
 *   per-scan corners -> one corner set (host, fp64)             ilcc_fuse_corners
 *   bag -> fused corners                                        ilcc_bag_corners_all_scans
 *
 * tests/sequence_ref.py restates the message order, the unpack and the fusion in numpy; it is the specification.
 */
#ifndef ILCC_SEQUENCE_H_
#define ILCC_SEQUENCE_H_

#include "ilcc_hip.h"
#include "ilcc_ingest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 1. every message of a topic ------------------------------------------------------------------------------------------
 * The messages on `topic` whose connection carries `md5sum` (NULL: PointCloud2's; "*" on either side matches, the rule of
 * ilcc_bag_first_message).  ORDER: record time; equal times by the chunk's position in the file, then by the offset inside the
 * chunk.  Entry 0 is the message ilcc_bag_first_message returns.  open reads the index section and walks every chunk that holds
 * such a message ONCE, one inflated chunk at a time, keeping (time, chunk, offset, length) per message; read inflates the entry's
 * chunk unless it is the one read last, so reading in order inflates every chunk once more and never holds more than one.
 * Refusals are those of ilcc_bag_first_message, with its texts (ILCC_IO_ERROR: unreadable, not V2.0, unindexed, unknown
 * compression, malformed; ILCC_BAD_ARGUMENT "no message of that type on topic").  An iterator is not thread-safe. */
typedef struct ilcc_bag_topic ilcc_bag_topic;
int32_t ilcc_bag_topic_open(const char* bag_path, const char* topic, const char* md5sum, ilcc_bag_topic** it);
uint64_t ilcc_bag_topic_count(const ilcc_bag_topic* it);
/* the RECORD time (the time field of the message-data record: when rosbag received it), not the header stamp */
int32_t ilcc_bag_topic_time(const ilcc_bag_topic* it, uint64_t i, uint32_t* sec, uint32_t* nsec);
/* *msg_bytes = the message's size even when cap is too small (ILCC_CAPACITY, nothing copied; msg may be NULL with cap 0) */
int32_t ilcc_bag_topic_read(ilcc_bag_topic* it, uint64_t i, uint8_t* msg, uint64_t cap, uint64_t* msg_bytes);
void ilcc_bag_topic_close(ilcc_bag_topic* it);

/* ---- 2. K0b: a batch of messages unpacked in one go -------------------------------------------------------------------------
 * d_blob (device) holds the data[] of n_msgs messages, message m at byte src_offsets[m]; layouts[m] is its layout (what
 * ilcc_pointcloud2_parse gave; data_offset is not used).  Writes the packed float4 clouds back to back into d_xyzi and
 * offsets_out[0 .. n_msgs] (host; offsets_out[m] = first point of message m, offsets_out[n_msgs] = all points): the d_xyzi +
 * offsets layout of ilcc_extract_batch_device.  Byte for byte what ilcc_pointcloud2_unpack_device writes message by message: each
 * message takes the tiled or the byte path by K0's own rule, evaluated on d_blob + src_offsets[m].  At most five launches however
 * many messages (one per layout class present: point_step 16 / 32 / 48 / 64 tiled, everything else).  Asynchronous on hip_stream.
 *
 * The per-message table travels through memory the plan owns (page-locked host copy, device copy, one asynchronous upload on
 * hip_stream in front of the launches).  A plan serves one call at a time: a call first waits for the plan's previous call to
 * have finished on the device.  Destroy it only after its last call has finished.  layouts and src_offsets are read, and
 * offsets_out is written, before the call returns: the caller may change or free the three arrays at once.
 *
 * Refusals -- all on the host, nothing launched or copied, d_xyzi and offsets_out untouched: null pointers / more messages than the
 * plan holds / a layout whose steps or fields do not fit its data_bytes (ILCC_BAD_ARGUMENT); a big-endian message
 * (ILCC_BAD_ARGUMENT, K0's text); a message whose data runs past blob_bytes (ILCC_BAD_ARGUMENT); more points than cap_points
 * (ILCC_CAPACITY). */
typedef struct ilcc_unpack_plan ilcc_unpack_plan;
ilcc_unpack_plan* ilcc_unpack_plan_create(uint32_t max_msgs);   /* on the current device; NULL on failure (ilcc_last_error(NULL)) */
void ilcc_unpack_plan_destroy(ilcc_unpack_plan* plan);
int32_t ilcc_pointcloud2_unpack_batch_device(const void* d_blob, uint64_t blob_bytes, const ilcc_pointcloud2_layout* layouts,
                                             const uint64_t* src_offsets, uint32_t n_msgs, void* d_xyzi, uint64_t cap_points,
                                             uint64_t* offsets_out, ilcc_unpack_plan* plan, void* hip_stream);
/* kernel launches of the plan's last accepted call (0..5) */
uint32_t ilcc_unpack_plan_launches(const ilcc_unpack_plan* plan);

/* ---- 3. fusion of per-scan corners (host, fp64; csrc/sequence_host.cpp, plain C++ built with -ffp-contract=off) -------------
 * corners: n x (a b) x 3 float32; a x b is the corner lattice, corner (i, j) at index i b + j (outer index on the short board
 * axis: the layout of ilcc_result.corners with a = board_w - 1, b = board_h - 1).  accepted: n flags.
 *   1. S = the accepted scans in input order.  S empty: ILCC_BOARD_NOT_FOUND, n_corners = 0.  ref_scan = the first scan of S.
 *   2. every scan of S is aligned to ref_scan: of the four index variants -- as is, outer flipped (a - 1 - i), inner flipped
 *      (b - 1 - j), both -- the one with the least cost, cost = the sum over corners in index order, then x, y, z, of the squared
 *      fp64 difference, added one by one; a tie goes to the lower variant.  (The plane frame's eigenvector signs are arbitrary, so
 *      two scans of one board may number its corners from opposite ends; the reference's check_order_lidar exists for that.)
 *   3. m0 = the median per coordinate over S (fp64; even count: (lo + hi) / 2).
 *   4. d2_i = max over corners of ((dx dx + dy dy) + dz dz) to m0; scan i is USED iff d2_i <= gate gate.
 *   5. n_ok = |S|, n_used = used scans.  n_used == 0 or 2 n_used <= n_ok: ILCC_AMBIGUOUS, n_corners = 0, counts filled (the board
 *      moved, or no majority agrees).
 *   6. m1 = the same median over the used scans, rounded to fp32 = corners; spread_max = sqrt of the largest d2 of a used scan to
 *      (the rounded) m1; spread_rms = sqrt(sum of all used scans' corner distances squared / (n_used a b)).
 * One gating round only.  ILCC_BAD_ARGUMENT: null pointers, a or b < 1, a b > ILCC_MAX_CORNERS, gate not positive and finite,
 * or an ACCEPTED scan with a non-finite coordinate (non-accepted scans are never read).
 * used_out (n flags) and dist_out (n doubles: sqrt(d2_i) to m1 of every scan of S when the status is ILCC_OK, to m0 when it is
 * ILCC_AMBIGUOUS; -1 for scans outside S) may be NULL. */
typedef struct ilcc_fused_corners {
  int32_t status;
  int32_t n_scans, n_ok, n_used;
  int32_t ref_scan;            /* -1: none */
  int32_t n_corners;
  double spread_rms, spread_max;   /* m */
  float corners[ILCC_MAX_CORNERS * 3];
} ilcc_fused_corners;
int32_t ilcc_fuse_corners(const float* corners, const uint8_t* accepted, uint32_t n, uint32_t a, uint32_t b, double gate,
                          ilcc_fused_corners* out, uint8_t* used_out, double* dist_out);

/* ---- 4. the chain ---------------------------------------------------------------------------------------------------------- */
enum { ILCC_SEED_CLICK = 0, ILCC_SEED_AUTO = 1, ILCC_SEED_AUTO_PLANAR = 2 };
#define ILCC_SEQUENCE_AUTO_TRIES 8

typedef struct ilcc_sequence_params {
  uint32_t first;               /* first message of the topic that is taken (time order) */
  uint32_t stride;              /* every stride-th from there (0 is read as 1) */
  uint32_t max_scans;           /* at most this many (0: all) */
  int32_t accept_ambiguous;     /* != 0: a scan with status ILCC_AMBIGUOUS is accepted too */
  int32_t accept_low_coverage;  /* != 0: ILCC_FLAG_LOW_COVERAGE does not reject a scan */
  int32_t reserved0;
  double gate;                  /* m; <= 0: grid_length / 2 -- half a square separates the true basin from its neighbour */
  uint64_t staging_bytes;       /* message data per batch; 0: 256 MiB */
} ilcc_sequence_params;

typedef struct ilcc_sequence_result {
  int32_t status;
  int32_t n_scans, n_ok, n_used;
  int32_t ref_scan;             /* index among the scans that ran (per_scan_out's index); -1: none */
  int32_t n_corners;
  double spread_rms, spread_max;
  float click[3];               /* the seed every scan ran with */
  int32_t n_batches;
  float corners[ILCC_MAX_CORNERS * 3];
} ilcc_sequence_result;

typedef struct ilcc_scan_record {
  ilcc_result result;
  uint32_t message;             /* index of the message on the topic */
  uint32_t stamp_sec, stamp_nsec;   /* the cloud's header stamp */
  uint32_t time_sec, time_nsec;     /* its record time */
  int32_t accepted, used;
  int32_t reserved0;
  double distance;              /* ilcc_fuse_corners' dist_out */
} ilcc_scan_record;

void ilcc_default_sequence_params(ilcc_sequence_params* sp);

/* Every selected scan of `topic` through the handle's pipeline with ONE click, then ilcc_fuse_corners on the accepted scans
 * (accept rule of ilcc_hip.h: status ILCC_OK and ILCC_FLAG_LOW_COVERAGE clear, each part switchable).
 * A batch is as many consecutive selected scans as fit the handle's max_frames, its max_total_points and staging_bytes; a single
 * scan above the handle's limits is ILCC_CAPACITY.  Per batch: the messages' data[] are staged in one page-locked blob at 16-byte
 * aligned offsets, one H2D copy, K0b, ilcc_submit_batch_device; the next batch is read, inflated, staged, copied and unpacked
 * while the pipeline works on this one (two sets of buffers, allocated once per call).
 * seed_mode ILCC_SEED_CLICK needs click; ILCC_SEED_AUTO / _AUTO_PLANAR run ilcc_extract_auto[_planar] (default seed parameters)
 * on the selected scans one at a time, at most the first ILCC_SEQUENCE_AUTO_TRIES, and take the first accepted scan's seed as
 * the click for all (the handle must hold max_seeds frames of such a scan, see ilcc_seed.h); none accepted:
 * ILCC_BOARD_NOT_FOUND.  No handle batch may be in flight.
 * per_scan_out (cap records; may be NULL): one record per scan that ran; fewer than the selected scans: ILCC_CAPACITY with
 * out->n_scans = the number needed, nothing run.
 * Returns out->status: ILCC_OK, ILCC_AMBIGUOUS / ILCC_BOARD_NOT_FOUND of the fusion (per_scan_out is complete then), or the
 * failure of a layer below. */
int32_t ilcc_bag_corners_all_scans(ilcc_handle* h, const char* bag_path, const char* topic, const float* click, int32_t seed_mode,
                                   const ilcc_sequence_params* sp, ilcc_sequence_result* out, ilcc_scan_record* per_scan_out,
                                   uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif
