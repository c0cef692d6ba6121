// What K13 (csrc/k13_jpeg.hip) and K14 (csrc/k14_jpeg_write.hip) share: EIGHT lanes own one 8 x 8 block, a row each, and turn
// rows into columns among themselves in registers -- three butterfly stages (lane ^ 1, ^ 2, ^ 4), the first two DPP quad
// permutes (VALU rate, no LDS pipe), the third a ds_swizzle -- and the 2- and 3-dword accesses at 4-byte aligned addresses.
#ifndef ILCC_JPEG_BLOCK8_H_
#define ILCC_JPEG_BLOCK8_H_

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ilcc {

struct alignas(4) Dword2 {
  uint32_t x, y;
};
struct alignas(4) Dword3 {
  uint32_t x, y, z;
};

// the value lane (l ^ S) holds, S = 1, 2 or 4
template <int S>
__device__ __forceinline__ int32_t lane_xor(int32_t x) {
  if constexpr (S == 1) return __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true);        // quad_perm [1, 0, 3, 2]
  else if constexpr (S == 2) return __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true);   // quad_perm [2, 3, 0, 1]
  else return __builtin_amdgcn_ds_swizzle(x, 0x101F);                                          // bit mode: and 0x1f, or 0, xor 4
}

// one butterfly stage of the 8 x 8 transpose among eight lanes: the S x S blocks off the diagonal change places
template <int S>
__device__ __forceinline__ void transpose_stage(int32_t (&v)[8], bool upper) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (i & S) continue;
    const int32_t got = lane_xor<S>(upper ? v[i] : v[i | S]);
    if (upper) v[i] = got;
    else v[i | S] = got;
  }
}

// lane r of an aligned group of eight holds M[r][0..7] -> it holds M[0..7][r]
__device__ __forceinline__ void transpose8(int32_t (&v)[8], int lane8) {
  transpose_stage<1>(v, (lane8 & 1) != 0);
  transpose_stage<2>(v, (lane8 & 2) != 0);
  transpose_stage<4>(v, (lane8 & 4) != 0);
}

}  // namespace ilcc

#endif
