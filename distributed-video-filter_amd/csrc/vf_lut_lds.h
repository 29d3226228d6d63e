// vf_lut_lds.h — the table lookup of the per-byte table kernels (vf_lut.hip, vf_level.hip): a
// 768-byte table in LDS, byte c * 256 + v the output of value v in channel c, and a 16-B vector or
// a tile of them through it.  Device code; not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vf_internal.h"
#include "vf_stream.h"

namespace vf {

struct LutArg {
  uint32_t w[192];  // byte c * 256 + v: the output of value v in channel c
};

template <int LAYOUT>
struct LutLds;

template <>
struct LutLds<0> {
  static constexpr int kWords = 192;
  static __device__ __forceinline__ void stage(uint32_t *s, const LutArg &tab) {
    if (threadIdx.x < 192) s[threadIdx.x] = tab.w[threadIdx.x];
  }
  static __device__ __forceinline__ uint32_t at(const uint32_t *s, uint32_t idx) {
    return reinterpret_cast<const uint8_t *>(s)[idx];
  }
};

template <>
struct LutLds<1> {
  static constexpr int kWords = 768;
  static __device__ __forceinline__ void stage(uint32_t *s, const LutArg &tab) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t i = (uint32_t)k * kBlock + threadIdx.x;
      s[i] = (tab.w[i >> 2] >> (8 * (i & 3))) & 0xFF;
    }
  }
  static __device__ __forceinline__ uint32_t at(const uint32_t *s, uint32_t idx) { return s[idx]; }
};

__device__ __forceinline__ uint32_t mod3_inc(uint32_t c, uint32_t by) {  // (c + by) % 3 for c, by < 3
  c += by;
  return c >= 3 ? c - 3 : c;
}

// One 16-B vector through the table.  h[m] = the channel of its byte m (m = 0..2; byte p has
// channel h[p % 3]); ROT rotates that by a compile-time count.
template <bool C3, int LAYOUT, int ROT>
__device__ __forceinline__ u32x4 lut16(const uint32_t *s, u32x4 v, const uint32_t h[3]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // byte 0 = byte k of w[j], byte 1 = the channel, bytes 2 and 3 zero
      const uint32_t idx = __builtin_amdgcn_perm(C3 ? h[(4 * j + k + ROT) % 3] : 0u, w[j], 0x0C0C0400u | (uint32_t)k);
      r |= LutLds<LAYOUT>::at(s, idx) << (8 * k);
    }
    o[j] = r;
  }
  u32x4 out;
  out.x = o[0];
  out.y = o[1];
  out.z = o[2];
  out.w = o[3];
  return out;
}

template <bool C3, int LAYOUT, int U, int J = 0>
__device__ __forceinline__ void lut_tile(const uint32_t *s, const u32x4 (&v)[U], u32x4 *d, const uint32_t h[3]) {
  if constexpr (J < U) {
    st16<true>(d + J * kBlock, lut16<C3, LAYOUT, J % 3>(s, v[J], h));
    lut_tile<C3, LAYOUT, U, J + 1>(s, v, d, h);
  }
}

template <bool C3, int LAYOUT, int U, int J = 0>
__device__ __forceinline__ void lut_partial(const uint32_t *s, const u32x4 *src, u32x4 *dst, uint64_t i0, uint64_t n16,
                                            const uint32_t h[3]) {
  if constexpr (J < U) {
    const uint64_t i = i0 + (uint64_t)J * kBlock;
    if (i < n16) st16<true>(dst + i, lut16<C3, LAYOUT, J % 3>(s, ld16<true>(src + i), h));
    lut_partial<C3, LAYOUT, U, J + 1>(s, src, dst, i0, n16, h);
  }
}
}  // namespace vf
