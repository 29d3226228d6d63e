// vf_binary.hip — the two-input per-byte arithmetic kernel of a filter chain (vf_chain_plan.h):
// dst[i] = op(a[i], b[i]) on uint8, op one of cv2.subtract (max(a - b, 0)), cv2.add
// (min(a + b, 255)), cv2.absdiff, cv2.min, cv2.max.  With it a chain expresses the morphological
// gradient, top-hat, black-hat and a difference of two blurs.
//
// The memory side is the table kernel's (vf_lut.hip): 16 B per lane per access, U = 4 vectors
// of each operand in flight, nontemporal loads and stores, grid-stride over whole tiles, head and
// tail bytes done bytewise by block 0.
//   * The 16-B grid is dst's: the body starts at dst's first 16-B boundary, so every body store is
//     one aligned nontemporal 16-B store.  a and b may each sit at any other offset mod 16 and are
//     read through load16_any (vf_tile.h), which is one nontemporal 16-B load when the operand
//     shares dst's alignment -- the case a chain produces -- and dword or byte loads otherwise.
//   * A byte is read and written by the same lane, the reads first, so dst == a or dst == b
//     exactly is allowed; partial overlap is the caller's to refuse (vf_binary_device does).
//   * gfx950 has no per-byte SIMD add / subtract / min / max, so the four bytes of a dword are
//     zero-extended into two pairs of 16-bit halves (v_perm_b32), combined with packed 16-bit ops
//     (v_pk_sub_u16 with clamp, v_pk_add_u16, v_pk_min_u16, v_pk_max_u16) and packed back by one
//     more v_perm_b32.
// Nothing is written outside [dst, dst + nbytes).  No device allocation; the launch stays
// asynchronous on the caller's stream.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "vf_internal.h"
#include "vf_stream.h"
#include "vf_tile.h"

namespace vf {

namespace {

using tile::load16_any;

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

enum : int { kSubtract = 0, kAdd = 1, kAbsdiff = 2, kMin = 3, kMax = 4 };  // VF_BIN_* (include/vfilter.h)

template <int OP>
__device__ __forceinline__ us2 op2(us2 x, us2 y) {  // on two values of 0..255 in 16-bit halves
  if constexpr (OP == kSubtract) return __builtin_elementwise_sub_sat(x, y);
  else if constexpr (OP == kAdd) return __builtin_elementwise_min(x + y, us2{255, 255});
  else if constexpr (OP == kAbsdiff) return __builtin_elementwise_max(x, y) - __builtin_elementwise_min(x, y);
  else if constexpr (OP == kMin) return __builtin_elementwise_min(x, y);
  else return __builtin_elementwise_max(x, y);
}

template <int OP>
__device__ __forceinline__ uint32_t op4(uint32_t x, uint32_t y) {  // on the four bytes of a dword
  // bytes 0, 1 and bytes 2, 3 zero-extended into the halves of a dword
  const us2 xl = __builtin_bit_cast(us2, __builtin_amdgcn_perm(0u, x, 0x0C010C00u));
  const us2 xh = __builtin_bit_cast(us2, __builtin_amdgcn_perm(0u, x, 0x0C030C02u));
  const us2 yl = __builtin_bit_cast(us2, __builtin_amdgcn_perm(0u, y, 0x0C010C00u));
  const us2 yh = __builtin_bit_cast(us2, __builtin_amdgcn_perm(0u, y, 0x0C030C02u));
  const us2 rl = op2<OP>(xl, yl), rh = op2<OP>(xh, yh);
  // the low bytes of the four halves as the four bytes of a dword
  return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, rh), __builtin_bit_cast(uint32_t, rl), 0x06040200u);
}

template <int OP>
__device__ __forceinline__ u32x4 op16(u32x4 x, u32x4 y) {
  u32x4 r;
  r.x = op4<OP>(x.x, y.x);
  r.y = op4<OP>(x.y, y.y);
  r.z = op4<OP>(x.z, y.z);
  r.w = op4<OP>(x.w, y.w);
  return r;
}

template <int OP>
__device__ __forceinline__ uint8_t op1(uint32_t x, uint32_t y) {
  if constexpr (OP == kSubtract) return (uint8_t)(x > y ? x - y : 0u);
  else if constexpr (OP == kAdd) return (uint8_t)(x + y > 255u ? 255u : x + y);
  else if constexpr (OP == kAbsdiff) return (uint8_t)(x > y ? x - y : y - x);
  else if constexpr (OP == kMin) return (uint8_t)(x < y ? x : y);
  else return (uint8_t)(x > y ? x : y);
}

// Body: n16 vectors of 16 B at a / b / dst, dst 16-B aligned, a and b at any alignment.
// Head / tail: up to 15 bytes each, bytewise by block 0.
template <int OP, int U>
__global__ __launch_bounds__(kBlock) void binary_kernel(
    const uint8_t *a, const uint8_t *b, u32x4 *dst, uint64_t n16,
    const uint8_t *ha, const uint8_t *hb, uint8_t *hdst, uint32_t head,
    const uint8_t *ta, const uint8_t *tb, uint8_t *tdst, uint32_t tail) {
  constexpr uint64_t TILE = (uint64_t)kBlock * U;
  const uint64_t stride = (uint64_t)gridDim.x * TILE;
  const uint32_t t = threadIdx.x;
  uint64_t t0 = (uint64_t)blockIdx.x * TILE;  // wave-uniform tile start
  for (; t0 + TILE <= n16; t0 += stride) {
    const uint64_t i0 = t0 + t;
    u32x4 x[U], y[U];
#pragma unroll
    for (int j = 0; j < U; ++j) x[j] = load16_any(a + ((i0 + (uint64_t)j * kBlock) << 4));
#pragma unroll
    for (int j = 0; j < U; ++j) y[j] = load16_any(b + ((i0 + (uint64_t)j * kBlock) << 4));
#pragma unroll
    for (int j = 0; j < U; ++j) st16<true>(dst + i0 + (uint64_t)j * kBlock, op16<OP>(x[j], y[j]));
  }
  if (t0 < n16) {  // the single partial tile, owned by whichever block reaches it
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const uint64_t i = t0 + (uint64_t)j * kBlock + t;
      if (i < n16) st16<true>(dst + i, op16<OP>(load16_any(a + (i << 4)), load16_any(b + (i << 4))));
    }
  }
  if (blockIdx.x == 0) {
    if (t < head) hdst[t] = op1<OP>(ha[t], hb[t]);
    if (t < tail) tdst[t] = op1<OP>(ta[t], tb[t]);
  }
}

template <int OP>
hipError_t launch_op(const uint8_t *a, const uint8_t *b, uint8_t *dst, size_t nbytes, int max_blocks,
                     hipStream_t stream) {
  constexpr int U = 4;
  const stream::Split s = stream::split(dst, nbytes);  // the 16-B grid is dst's
  const size_t t = s.tail_at();
  hipLaunchKernelGGL((binary_kernel<OP, U>), dim3(stream::blocks(s.n16, (uint64_t)kBlock * U, max_blocks)), dim3(kBlock),
                     0, stream, a + s.head, b + s.head, reinterpret_cast<u32x4 *>(dst + s.head), s.n16, a, b, dst, s.head,
                     a + t, b + t, dst + t, s.tail);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_binary(const void *da, const void *db, void *ddst, size_t nbytes, int op, const LaunchCfg &cfg,
                         hipStream_t stream) {
  if (nbytes == 0) return hipSuccess;
  if (!da || !db || !ddst || cfg.max_blocks < 1) return hipErrorInvalidValue;
  const uint8_t *a = static_cast<const uint8_t *>(da), *b = static_cast<const uint8_t *>(db);
  uint8_t *dst = static_cast<uint8_t *>(ddst);
  switch (op) {
    case kSubtract: return launch_op<kSubtract>(a, b, dst, nbytes, cfg.max_blocks, stream);
    case kAdd: return launch_op<kAdd>(a, b, dst, nbytes, cfg.max_blocks, stream);
    case kAbsdiff: return launch_op<kAbsdiff>(a, b, dst, nbytes, cfg.max_blocks, stream);
    case kMin: return launch_op<kMin>(a, b, dst, nbytes, cfg.max_blocks, stream);
    case kMax: return launch_op<kMax>(a, b, dst, nbytes, cfg.max_blocks, stream);
  }
  return hipErrorInvalidValue;
}

}  // namespace vf
