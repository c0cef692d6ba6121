/*
 * ilcc_jpeg.h -- reading JPEG images: the camera half of the reference runs through .jpg files
 * (get_image_corners_bag.cpp:110 writes process_data/<camera><i>.jpg, libcbdetect/demo_all_pic.m:8-19 and
 * calib_lidar_cam.cpp:108,128 read them), and a camera bag recorded the usual way carries
 * sensor_msgs/CompressedImage.  Implemented in libilcc_hip.so: headers and Huffman decoding on the host
 * (csrc/jpeg_entropy.cpp, plain C++ without HIP), everything from coefficients to pixels on the GPU (K13,
 * csrc/k13_jpeg.hip), the chained entries in csrc/jpeg_host.cpp.
 *
 *   reference                                                   here
 *   ----------------------------------------------------------  ------------------------------------
 *   cv::imread / MATLAB imread of <camera><i>.jpg                ilcc_jpeg_decode_device
 *   demo_all_pic.m on one file (imread -> findCorners ->         ilcc_jpeg_find_chessboard
 *     chessboardsFromCorners -> <camera><i>.txt)
 *   cv_bridge::toCvCopy of a sensor_msgs/CompressedImage         ilcc_compressed_image_parse + ilcc_jpeg_decode_device;
 *                                                                the ilcc_bag_* entries take it by themselves
 *
 * Accepted: baseline and extended sequential frames (SOF0, SOF1) with 8-bit samples and Huffman coding, one scan
 * holding all components, restart intervals, optimised Huffman tables, APPn / COM segments (skipped); 1 component, or
 * 3 components taken as Y, Cb, Cr with luma sampled 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) and both chroma 1x1.
 * Refused with ILCC_BAD_ARGUMENT and a last-error text that names the cause: progressive, lossless and arithmetic
 * frames, 12-bit samples, 16-bit quantisation tables, 2 or 4 components, Adobe APP14 with transform 0 on 3
 * components, other sampling factors, several scans, DNL, a table used before it is defined, a Huffman code in no
 * table, a run past coefficient 63, a DC predictor that leaves int16, data that ends early, a width or height of 0.
 *
 * The arithmetic is libjpeg's default path (jidctint "islow", "fancy" upsampling, jdcolor), which cv::imread,
 * MATLAB's imread and Pillow share; tests/jpeg_ref.py restates it in numpy.  All of it is int32 with arithmetic
 * shifts, DESCALE(x, n) = (x + (1 << (n - 1))) >> n.
 *   sample block = clamp(IDCT(coef * quant) + 128, 0, 255); pass 1 over COLUMNS with DESCALE by 11, pass 2 over
 *   rows with DESCALE by 18 (rounding does not commute).  With c0..c7 the inputs of a pass:
 *     z1 = (c2+c6)*4433;  t2 = z1 - c6*15137;  t3 = z1 + c2*6270;  t0 = (c0+c4) << 13;  t1 = (c0-c4) << 13
 *     t10 = t0+t3; t13 = t0-t3; t11 = t1+t2; t12 = t1-t2;   o0 = c7; o1 = c5; o2 = c3; o3 = c1
 *     z1 = o0+o3; z2 = o1+o2; z3 = o0+o2; z4 = o1+o3; z5 = (z3+z4)*9633
 *     o0 *= 2446; o1 *= 16819; o2 *= 25172; o3 *= 12299
 *     z1 *= -7373; z2 *= -20995; z3 = z3*(-16069) + z5; z4 = z4*(-3196) + z5
 *     o0 += z1+z3; o1 += z2+z4; o2 += z2+z3; o3 += z1+z4
 *     out0..7 = t10+o3, t11+o2, t12+o1, t13+o0, t13-o0, t12-o1, t11-o2, t10-o3
 *   libjpeg's C code works in 64-bit long and its SIMD code in 32-bit lanes; they agree while no intermediate
 *   leaves int32, which holds for every file an encoder made.  Outside that domain the bytes are unspecified
 *   (the kernel still writes only inside the image).
 *   chroma plane of real size wc x hc (wc = ceil(w / 2) where luma is sampled twice as densely), s[] clamped to
 *   the real samples at every edge:
 *     2x1:  out[2i] = (3 s[i] + s[i-1] + 1) >> 2;   out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2
 *     2x2:  r[2j] = 3 s[j] + s[j-1], r[2j+1] = 3 s[j] + s[j+1] down each column, then along the row
 *           out[2i] = (3 r[i] + r[i-1] + 8) >> 4;   out[2i+1] = (3 r[i] + r[i+1] + 7) >> 4
 *     as libjpeg does, a plane with wc <= 2 is replicated instead (out[x] = s[x / 2], rows likewise).
 *   colour, cb -= 128, cr -= 128:  R = Y + ((91881 cr + 32768) >> 16);  B = Y + ((116130 cb + 32768) >> 16);
 *     G = Y + ((-22554 cb - 46802 cr + 32768) >> 16); each clamped to 0..255 and stored B, G, R.
 *
 * Not here: progressive JPEG, PNG.
 */
#ifndef ILCC_JPEG_H_
#define ILCC_JPEG_H_

#include <stdint.h>

#include "ilcc_camera_image.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ilcc_jpeg_component {
  int32_t h, v;                 /* sampling factors; 1, 1 for a single component (its scan is not interleaved) */
  int32_t quant_index;          /* row of ilcc_jpeg_info.quant */
  int32_t dc_table, ac_table;   /* Huffman table indices of the scan */
  int32_t blocks_w, blocks_h;   /* 8 x 8 blocks, padded to whole MCUs */
  int32_t reserved;
  uint64_t coef_offset;         /* of the component's first block in the coefficient buffer, in int16 */
} ilcc_jpeg_component;

typedef struct ilcc_jpeg_info {
  int32_t width, height;
  int32_t n_components;         /* 1 or 3 */
  int32_t restart_interval;     /* MCUs between RSTn markers, 0: none */
  ilcc_jpeg_component comp[3];
  uint16_t quant[4][64];        /* natural (row-major) order */
  uint64_t coef_count;          /* int16 in the coefficient buffer: 64 per block of every component */
  uint64_t scan_offset;         /* of the first entropy-coded byte */
} ilcc_jpeg_info;

/* Headers only, up to the start of the scan.  Allocates nothing; never reads past `bytes`.  Host only. */
int32_t ilcc_jpeg_parse(const uint8_t* jpg, uint64_t bytes, ilcc_jpeg_info* out);

/* blocks_w, blocks_h, coef_offset of every component and coef_count from width, height, n_components and h, v (for
 * coefficients that come from elsewhere than a file).  ILCC_BAD_ARGUMENT for a size outside 1 .. 65535 or a sampling
 * outside the accepted set. */
int32_t ilcc_jpeg_layout(ilcc_jpeg_info* info);

/* The quantised coefficients of the scan, de-zigzagged: coef[coef_offset_c + (by * blocks_w_c + bx) * 64 + k], k
 * row-major in the block; blocks that pad the image to whole MCUs are decoded like any other, and `cap` int16 must
 * hold info->coef_count (ILCC_CAPACITY).  Handles byte stuffing and RSTn (predictors reset, the markers must come
 * in order).  `info` is what ilcc_jpeg_parse made of the same bytes.  Allocates nothing.  Host only. */
int32_t ilcc_jpeg_entropy_decode(const uint8_t* jpg, uint64_t bytes, const ilcc_jpeg_info* info, int16_t* coef, uint64_t cap);

/* Bytes of device scratch K13 needs for `info`: the three padded sample planes of a colour image, 0 for 1 component
 * (and for an info ilcc_jpeg_layout would refuse). */
uint64_t ilcc_jpeg_scratch_bytes(const ilcc_jpeg_info* info);

/* K13: coefficients in device memory (16-byte aligned, laid out as above) -> pixels in device memory, rows dst_stride
 * bytes apart: mono8 for 1 component, bgr8 for 3.  Two kernels: k13_idct (dequantise, inverse DCT, +128, clamp; a
 * 1-component image straight into d_dst, clipped at the right and bottom edge; a 3-component image into the planes in
 * d_scratch) and k13_upsample_colour (planes -> B, G, R).  Not a byte outside [row * dst_stride, row * dst_stride +
 * bpp * width) is written.  Asynchronous on hip_stream; info is read before the call returns.  Checked on the host
 * before any launch (ILCC_BAD_ARGUMENT): null pointers, an info whose block counts or offsets are not
 * ilcc_jpeg_layout's, a stride shorter than a row, a misaligned d_coef, scratch_bytes < ilcc_jpeg_scratch_bytes. */
int32_t ilcc_jpeg_idct_device(const ilcc_jpeg_info* info, const int16_t* d_coef, void* d_dst, int32_t dst_stride, void* d_scratch,
                              uint64_t scratch_bytes, void* hip_stream);

/* parse -> entropy decode -> upload -> K13 on the current device, one hipMalloc / hipFree for coefficients and scratch.
 * *width, *height and *encoding (ILCC_ENCODING_MONO8 or ILCC_ENCODING_BGR8: the file's own) are set whenever the
 * headers parse; cap_bytes < (height - 1) * dst_stride + bpp * width is ILCC_CAPACITY with nothing written.  The
 * kernels run on hip_stream; the call waits for that stream before it returns (its coefficient buffer is freed on return), so
 * `jpg` has been read and the pixels are in d_dst when it does. */
int32_t ilcc_jpeg_decode_device(const uint8_t* jpg, uint64_t bytes, void* d_dst, int32_t dst_stride, uint64_t cap_bytes, int32_t* width,
                                int32_t* height, int32_t* encoding, void* hip_stream);

/* demo_all_pic.m on one file: file -> K13 -> K11 (mono8; undistorted only when a camera is given: the reference's
 * jpgs are already undistorted) -> K10.  rows, cols, xy as ilcc_find_chessboard_device. */
int32_t ilcc_jpeg_find_chessboard(int32_t device, const char* jpg_path, const ilcc_camera_model* camera_or_null, int32_t board_w,
                                  int32_t board_h, int32_t* rows, int32_t* cols, double* xy);

typedef struct ilcc_compressed_image_layout {
  uint32_t stamp_sec, stamp_nsec, seq;
  uint32_t reserved;
  uint64_t data_offset;         /* of data[] inside the serialized message */
  uint64_t data_bytes;
  char frame_id[64];
  char format[64];
} ilcc_compressed_image_layout;

/* layout of a serialized sensor_msgs/CompressedImage (md5sum 8f7a12909da2c9d3332d540a0977563f): header, format,
 * data[].  ILCC_BAD_ARGUMENT: a truncated message, a length field that runs past it, empty data, a format that holds
 * neither "jpeg" nor "jpg" (the last-error text names it).  Allocates nothing.  Host only. */
int32_t ilcc_compressed_image_parse(const uint8_t* msg, uint64_t msg_bytes, ilcc_compressed_image_layout* out);

#ifdef __cplusplus
}
#endif
#endif
