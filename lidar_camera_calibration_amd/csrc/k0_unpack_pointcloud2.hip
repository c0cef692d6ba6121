// K0 unpack_pointcloud2 -- replaces pcl::fromROSMsg(msg, pcl::PointCloud<pcl::PointXYZI>)
// (/root/reference/ilcc2/test/get_lidar_corners.cpp:163-164) for the device-resident path:
// sensor_msgs/PointCloud2 data[] (point_step bytes per point, row_step bytes per row) ->
// packed float4 {x, y, z, intensity}.  Unmatched fields stay 0 (pcl::PointXYZI's constructor zeroes them).
//
// HBM-bound: point_step bytes read + 16 bytes written per point (velodyne: 32 + 16).
//  * fast path (point_step % 16 == 0, field offsets % 4 == 0, base 16-byte aligned, rows packed):
//    a workgroup stages kTile points through LDS with 16-byte loads in memory order -- every lane of a
//    wavefront reads consecutive 16-byte pieces (1 KiB per wave-load, fully coalesced) -- then each
//    lane picks its point's four dwords out of LDS and writes one float4 (coalesced).
//  * generic path: four 4-byte reads per point assembled from bytes (any alignment, any padding).
// Launch: one workgroup of 256 threads per 1024 points -> 29 workgroups per VLP-16 message; a batch of
// messages is one launch (height := messages * height), >= 3.6k workgroups at 128 frames.
#include <hip/hip_runtime.h>

#include "host_util.h"
#include "ilcc_ingest.h"
#include "ilcc_internal.h"
#include "k0_unpack.h"   // the device code of a tile and of a generic point, shared with K0b

namespace ilcc {

__global__ __launch_bounds__(kUnpackThreads) void k0_unpack_generic(UnpackArgs a) {
  unpack_generic_point(a, (uint64_t)blockIdx.x * kUnpackThreads + threadIdx.x);
}

template <int STEP16>
__global__ __launch_bounds__(kUnpackThreads) void k0_unpack_tiled(UnpackArgs a) {
  __shared__ u32x4 tile[kUnpackTile * STEP16];
  unpack_tile<STEP16>(a, (uint64_t)blockIdx.x * kUnpackTile, tile);
}

}  // namespace ilcc

extern "C" int32_t ilcc_pointcloud2_unpack_device(const void* d_data, const ilcc_pointcloud2_layout* L, void* d_xyzi,
                                                  void* hip_stream) {
  using namespace ilcc;
  if (!L || (!d_data && L->data_bytes) || !d_xyzi) return fail(ILCC_BAD_ARGUMENT, "null argument");
  // pcl::fromROSMsg memcpy's fields: it is wrong on such data too; refuse instead
  if (L->is_bigendian) return fail(ILCC_BAD_ARGUMENT, "big-endian PointCloud2 is not supported");
  UnpackArgs a;
  unpack_args_from_layout(*L, d_data, d_xyzi, &a);
  if (a.n_points == 0) return ILCC_OK;
  hipStream_t s = (hipStream_t)hip_stream;
  const int cls = unpack_class(*L, d_data);
  if (cls) {
    const uint32_t blocks = (uint32_t)((a.n_points + kUnpackTile - 1) / kUnpackTile);
    switch (cls) {
      case 1: hipLaunchKernelGGL(k0_unpack_tiled<1>, dim3(blocks), dim3(kUnpackThreads), 0, s, a); break;
      case 2: hipLaunchKernelGGL(k0_unpack_tiled<2>, dim3(blocks), dim3(kUnpackThreads), 0, s, a); break;
      case 3: hipLaunchKernelGGL(k0_unpack_tiled<3>, dim3(blocks), dim3(kUnpackThreads), 0, s, a); break;
      default: hipLaunchKernelGGL(k0_unpack_tiled<4>, dim3(blocks), dim3(kUnpackThreads), 0, s, a); break;
    }
  } else {
    const uint32_t blocks = (uint32_t)((a.n_points + kUnpackThreads - 1) / kUnpackThreads);
    hipLaunchKernelGGL(k0_unpack_generic, dim3(blocks), dim3(kUnpackThreads), 0, s, a);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ILCC_HIP_ERROR, std::string("k0 launch: ") + hipGetErrorString(e));
  return ILCC_OK;
}

extern "C" int32_t ilcc_bag_first_cloud(int32_t device, const char* bag_path, const char* topic, float* xyzi,
                                        uint32_t cap_points, uint32_t* n_points) {
  using namespace ilcc;
  if (!n_points || (!xyzi && cap_points)) return fail(ILCC_BAD_ARGUMENT, "null argument");
  *n_points = 0;
  std::vector<uint8_t> msg;
  int32_t st = read_first_message(bag_path, topic, nullptr, &msg);
  if (st != ILCC_OK) return st;
  ilcc_pointcloud2_layout L;
  st = ilcc_pointcloud2_parse(msg.data(), msg.size(), &L);
  if (st != ILCC_OK) return st;
  const uint64_t pts = (uint64_t)L.height * L.width;
  *n_points = (uint32_t)pts;
  if (pts > cap_points) return fail(ILCC_CAPACITY, "cloud larger than the buffer");
  if (pts == 0) return ILCC_OK;
  st = select_device(device);
  if (st != ILCC_OK) return st;
  DeviceBuffer in, out;
  hipError_t e = hipMalloc(&in.p, L.data_bytes);
  if (e == hipSuccess) e = hipMalloc(&out.p, pts * 16);
  if (e == hipSuccess) e = hipMemcpy(in.p, msg.data() + L.data_offset, L.data_bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e);
  st = ilcc_pointcloud2_unpack_device(in.p, &L, out.p, nullptr);
  if (st != ILCC_OK) return st;
  e = hipMemcpy(xyzi, out.p, pts * 16, hipMemcpyDeviceToHost);
  return e == hipSuccess ? ILCC_OK : hip_fail(e);
}
