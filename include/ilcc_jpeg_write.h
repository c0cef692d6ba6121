/*
 * ilcc_jpeg_write.h -- writing JPEG images: get_image_corners_bag ends each bag with
 * cv::imwrite(process_data/<camera><i>.jpg, rectifyImage) (get_image_corners_bag.cpp:104-110), and MATLAB's
 * demo_all_pic.m and calib_lidar_cam read those files back.  This is that imwrite: libjpeg's encoder with its defaults
 * (baseline, Annex-K tables scaled by the quality, standard Huffman tables, 4:2:0 for colour), byte for byte.
 * Implemented in libilcc_hip.so and split like the reader (ilcc_jpeg.h): everything that is independent per pixel or
 * per block on the GPU (K14, csrc/k14_jpeg_write.hip: colour conversion, chroma downsampling, level shift, forward DCT,
 * quantisation), the Huffman coding, one serial bit stream, on the host (csrc/jpeg_entropy_enc.cpp, plain C++ without
 * HIP), the chained entries in csrc/jpeg_write_host.cpp.
 *
 *   reference                                                   here
 *   ----------------------------------------------------------  ------------------------------------
 *   cv::imwrite(<camera><i>.jpg, image)                          ilcc_jpeg_write_file / ilcc_jpeg_encode_device
 *   the per-bag body of get_image_corners_bag (first image ->    ilcc_bag_save_jpeg
 *     undistort -> imwrite)
 *
 * The coefficient buffer is the reader's: coef[coef_offset_c + (by * blocks_w_c + bx) * 64 + k], k row-major in the
 * block, blocks padded to whole MCUs (ilcc_jpeg_entropy_decode).  ilcc_jpeg_entropy_decode(ilcc_jpeg_entropy_encode(c))
 * == c for every encodable c.
 *
 * The arithmetic is libjpeg's default forward path (jccolor, the plain h2v1 / h2v2 downsamplers, jfdctint "islow" and
 * its quantiser), which cv::imwrite and Pillow share; tests/jpeg_write_ref.py restates it in numpy.  All of it is int32
 * with arithmetic shifts, D(x) = (x + (1 << (s - 1))) >> s.
 *   quantisation tables: quality clamped to 1 .. 100; scale = q < 50 ? 5000 / q : 200 - 2 q;
 *     quant[k] = clamp((std[k] * scale + 50) / 100, 1, 255), std the Annex-K luminance (table 0) or chrominance (table 1).
 *   colour, from B, G, R:
 *     Y  = ( 19595 R + 38470 G +  7471 B +   32768) >> 16
 *     Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16
 *     Cr = ( 32768 R - 27439 G -  5329 B + 8421375) >> 16
 *   chroma downsampling, by output column i:   2x1: (a + b + (i & 1)) >> 1;   2x2: (a + b + c + d + 1 + (i & 1)) >> 2
 *   padding to the component's REAL block grid (ceil(real size / 8) blocks each way).  It is asymmetric:
 *     full-resolution COLUMNS are replicated BEFORE downsampling, so a padded chroma column is the rounded mean of the
 *       last pixel column, with its own bias;
 *     an odd last row is replicated once to complete its pair; below that, DOWNSAMPLED rows are replicated.
 *     For luma, and for a 1-component image, this is: column and row indices clamped to the image.
 *   sample block - 128 -> jfdctint: pass 1 over ROWS, pass 2 over columns.  One pass over d0 .. d7:
 *     t0=d0+d7 t7=d0-d7 t1=d1+d6 t6=d1-d6 t2=d2+d5 t5=d2-d5 t3=d3+d4 t4=d3-d4
 *     t10=t0+t3 t13=t0-t3 t11=t1+t2 t12=t1-t2
 *     pass 1: o0=(t10+t11)<<2  o4=(t10-t11)<<2  s=11;   pass 2: o0=(t10+t11+2)>>2  o4=(t10-t11+2)>>2  s=15
 *     z1=(t12+t13)*4433  o2=D(z1+t13*6270)  o6=D(z1-t12*15137)
 *     z1=t4+t7 z2=t5+t6 z3=t4+t6 z4=t5+t7 z5=(z3+z4)*9633
 *     t4*=2446 t5*=16819 t6*=25172 t7*=12299  z1*=-7373 z2*=-20995 z3=z3*(-16069)+z5 z4=z4*(-3196)+z5
 *     o7=D(t4+z1+z3) o5=D(t5+z2+z4) o3=D(t6+z2+z3) o1=D(t7+z1+z4)
 *   quantisation: d = 8 * quant[k], q = sign(c) * ((|c| + (d >> 1)) / d).
 *   blocks that pad an interleaved scan to whole MCUs are libjpeg's dummy blocks, not transformed padding: all AC zero;
 *     a block right of the component's real blocks takes the DC of the block to its left, a block below them the DC of
 *     the previous block in MCU order (4:2:0 luma: both blocks of the dummy row take the DC of the MCU's top-right
 *     block).  With the accepted samplings only luma has them: at most one column and one row.
 *
 * Not here: optimised Huffman tables, progressive or arithmetic output, input encodings other than mono8 and bgr8.
 */
#ifndef ILCC_JPEG_WRITE_H_
#define ILCC_JPEG_WRITE_H_

#include <stdint.h>

#include "ilcc_jpeg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The info of a file to write: size, components (1, or 3 = Y, Cb, Cr with luma sampled sampling_h x sampling_v: 1x1,
 * 2x1 or 2x2; ignored for 1 component), Huffman and quantisation indices (luma 0, chroma 1), quant[0..1] from `quality`
 * as above, the restart interval in MCUs (0: none), and the layout by ilcc_jpeg_layout.  scan_offset is 0.
 * ILCC_BAD_ARGUMENT: a size outside 1 .. 65535, components other than 1 or 3, a sampling outside the accepted set, a
 * restart interval outside 0 .. 65535.  Host only. */
int32_t ilcc_jpeg_write_info(int32_t width, int32_t height, int32_t n_components, int32_t sampling_h, int32_t sampling_v,
                             int32_t quality, int32_t restart_interval, ilcc_jpeg_info* out);

/* Bytes of device scratch K14 needs for `info`: the padded Y, Cb, Cr sample planes of a colour image, 0 for 1 component
 * (and for an info ilcc_jpeg_layout would refuse). */
uint64_t ilcc_jpeg_fdct_scratch_bytes(const ilcc_jpeg_info* info);

/* K14: pixels in device memory (ILCC_ENCODING_MONO8 for 1 component, ILCC_ENCODING_BGR8 for 3; rows src_stride bytes
 * apart) -> info->coef_count int16 in device memory (16-byte aligned), in exactly the decoder's layout, dummy blocks
 * included.  Two kernels: k14_colour_downsample (3 components only: B, G, R -> the padded planes in d_scratch) and
 * k14_fdct_quant (once per component).  Nothing is read outside [row * src_stride, row * src_stride + bpp * width) of
 * the source, nothing written outside the coef_count coefficients.  Asynchronous on hip_stream; info is read before
 * the call returns.  Checked on the host before any launch (ILCC_BAD_ARGUMENT): null pointers, an info whose block
 * counts or offsets are not ilcc_jpeg_layout's or that holds a quantisation entry outside 1 .. 255, a stride shorter
 * than a row, an encoding that does not fit the component count, a misaligned d_coef, scratch_bytes <
 * ilcc_jpeg_fdct_scratch_bytes. */
int32_t ilcc_jpeg_fdct_device(const ilcc_jpeg_info* info, const void* d_src, int32_t src_stride, int32_t encoding, int16_t* d_coef,
                              void* d_scratch, uint64_t scratch_bytes, void* hip_stream);

/* A byte count no file for this info can exceed (0 for an info ilcc_jpeg_layout would refuse).  Host only. */
uint64_t ilcc_jpeg_file_bound(const ilcc_jpeg_info* info);

/* The whole file as libjpeg writes it: SOI; APP0 "JFIF\0" 01 01 00 0001 0001 00 00; one DQT segment per table used;
 * SOF0; one DHT segment per table (DC 0, AC 0, and for 3 components DC 1, AC 1: the Annex-K tables); DRI only when the
 * interval is non-zero; SOS; the scan; EOI.  In the scan: byte stuffing, 1-bits to pad before RSTn and at the end, RSTn
 * every restart_interval MCUs with the predictors reset.  `coef` holds info->coef_count int16; *bytes is the file's
 * size.  Allocates nothing and writes nothing past `cap` (ILCC_CAPACITY; what was written up to there is unspecified).
 * ILCC_BAD_ARGUMENT with the cause in the last-error text: a DC difference outside 11 bits, an AC value outside 10
 * bits (libjpeg refuses these too), an info that is not ilcc_jpeg_write_info's shape.  Host only. */
int32_t ilcc_jpeg_entropy_encode(const ilcc_jpeg_info* info, const int16_t* coef, uint8_t* out, uint64_t cap, uint64_t* bytes);

/* info -> K14 -> D2H -> entropy encode on the current device, one hipMalloc / hipFree for coefficients and scratch.
 * d_src: width x height pixels in device memory, ILCC_ENCODING_MONO8 or ILCC_ENCODING_BGR8 (then 3 components sampled
 * sampling_h x sampling_v; both are ignored for mono8).  Returns when the file's *bytes bytes are in `out` (host). */
int32_t ilcc_jpeg_encode_device(const void* d_src, int32_t src_stride, int32_t width, int32_t height, int32_t encoding, int32_t quality,
                                int32_t sampling_h, int32_t sampling_v, int32_t restart_interval, uint8_t* out, uint64_t cap,
                                uint64_t* bytes, void* hip_stream);

/* cv::imwrite(path, image) for host pixels: upload, encode, write the file; the counterpart of ilcc_save_ppm_bgr.
 * Colour is written 4:2:0, libjpeg's default and therefore imwrite's; no restart markers. */
int32_t ilcc_jpeg_write_file(int32_t device, const char* path, const uint8_t* pixels, int32_t stride, int32_t width, int32_t height,
                             int32_t encoding, int32_t quality);

/* The per-bag body of get_image_corners_bag: the topic's first Image (or CompressedImage) -> K11 (mono8, undistorted
 * with `camera`) -> K14 -> jpg_path.  One hipMalloc for the call; the pixels never visit the host. */
int32_t ilcc_bag_save_jpeg(int32_t device, const char* bag_path, const char* topic, const ilcc_camera_model* camera,
                           const char* jpg_path, int32_t quality);

#ifdef __cplusplus
}
#endif
#endif
