// vf_lut.hip — the 256-entry table filter on raw frames: dst[i] = table[channel(i)][src[i]],
// cv2.LUT(frame, table) for uint8 frames of 1 or 3 interleaved channels.  Every per-pixel
// filter of the reference's plugin slot (inverter.py:41) that is not bitwise_not -- gamma,
// levels, threshold, posterize, per-channel curves -- is one of these tables.
//
// The memory side is invert_stream_kernel's (vf_stream.h): 16 B per lane per access, U = 4
// independent loads in flight, nontemporal loads and stores, grid-stride over whole tiles, the
// head and tail bytes of an unaligned range done bytewise by block 0.  The filter itself is
// one LDS byte read per input byte:
//   * the table arrives BY VALUE as a kernel argument (768 B: three planar 256-byte tables, a
//     one-channel table stored three times), so a launch needs no device allocation, nothing
//     has a lifetime and the launch stays asynchronous on the caller's stream; each workgroup
//     copies it into LDS once, then runs its tiles;
//   * 16 = 1 (mod 3), so byte k of body vector i has channel (c0 + i + k) % 3 with c0 the
//     channel of the body's first byte; 256 = 1 (mod 3) too, so the U vectors of a lane's tile
//     are one rotation apart and a lane keeps three table offsets, rotated per vector at
//     compile time and advanced by (grid stride % 3) per tile;
//   * the LDS address of a lookup is (channel << 8 | byte), built by one v_perm_b32.
// LAYOUT (VF_LUT_LAYOUT in the environment, read once; for measurements): 0 = the table as it
// is, 768 B, four entries per LDS dword (the default: the faster of the two, at 99 % of the
// invert kernel's rate); 1 = one entry per dword, 3 KiB.  DESIGN.md 15 records what each
// measured, and what else was tried and dropped.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <cstring>

#include "vf_env.h"
#include "vf_internal.h"
#include "vf_lut_lds.h"
#include "vf_stream.h"

namespace vf {

namespace {

// Body: n16 aligned 16-B vectors at src/dst.  Head/tail: up to 15 bytes each, bytewise by block 0.
// phases: bits 0-1 the channel of the body's first byte, 2-3 of the head's, 4-5 of the tail's.
template <int U, bool C3, int LAYOUT>
__global__ __launch_bounds__(kBlock) void lut_stream_kernel(
    const u32x4 *__restrict__ src, u32x4 *__restrict__ dst, uint64_t n16,
    const uint8_t *__restrict__ hsrc, uint8_t *__restrict__ hdst, uint32_t head,
    const uint8_t *__restrict__ tsrc, uint8_t *__restrict__ tdst, uint32_t tail, uint32_t phases,
    const LutArg tab) {
  __shared__ uint32_t s[LutLds<LAYOUT>::kWords];
  LutLds<LAYOUT>::stage(s, tab);
  __syncthreads();
  constexpr uint64_t TILE = (uint64_t)kBlock * U;
  const uint64_t stride = (uint64_t)gridDim.x * TILE;
  const uint32_t t = threadIdx.x;
  uint64_t t0 = (uint64_t)blockIdx.x * TILE;  // wave-uniform tile start
  // the channel of byte 0 of this lane's first vector, and how far a grid stride moves it
  uint32_t c = C3 ? (uint32_t)(((phases & 3) + t0 + t) % 3) : 0;
  const uint32_t step = C3 ? (uint32_t)(stride % 3) : 0;
  for (; t0 + TILE <= n16; t0 += stride) {
    const u32x4 *sp = src + t0 + t;
    u32x4 v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) v[j] = ld16<true>(sp + j * kBlock);
    const uint32_t h[3] = {c, mod3_inc(c, 1), mod3_inc(c, 2)};
    lut_tile<C3, LAYOUT, U>(s, v, dst + t0 + t, h);
    c = mod3_inc(c, step);
  }
  if (t0 < n16) {  // the single partial tile, owned by whichever block reaches it
    const uint32_t h[3] = {c, mod3_inc(c, 1), mod3_inc(c, 2)};
    lut_partial<C3, LAYOUT, U>(s, src, dst, t0 + t, n16, h);
  }
  if (blockIdx.x == 0) {
    const uint32_t hc = C3 ? ((phases >> 2) & 3) + t : 0, tc = C3 ? ((phases >> 4) & 3) + t : 0;
    if (t < head) hdst[t] = (uint8_t)LutLds<LAYOUT>::at(s, (hc % 3) << 8 | hsrc[t]);
    if (t < tail) tdst[t] = (uint8_t)LutLds<LAYOUT>::at(s, (tc % 3) << 8 | tsrc[t]);
  }
}

// src and dst at different offsets mod 16: no common 16-B grid.  Bytewise, grid-stride; correct
// at any alignment and an order of magnitude slower than the stream kernel (callers that care
// keep the two congruent mod 16, as vf_lut_frames_host's staging does).
template <bool C3>
__global__ __launch_bounds__(kBlock) void lut_bytes_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                           uint64_t n, uint32_t phase, const LutArg tab) {
  __shared__ uint32_t s[LutLds<0>::kWords];
  LutLds<0>::stage(s, tab);
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const uint32_t c = C3 ? (uint32_t)((phase + i) % 3) : 0;
    dst[i] = (uint8_t)LutLds<0>::at(s, c << 8 | src[i]);
  }
}

template <bool C3, int LAYOUT>
hipError_t launch_lut_stream(const uint8_t *src, uint8_t *dst, size_t nbytes, uint32_t phase, const LutArg &tab,
                             int max_blocks, hipStream_t stream) {
  constexpr int U = 4;
  constexpr uint64_t TILE = (uint64_t)kBlock * U;
  // launch_stream's split and sub-launches, with the channel of each part's first byte beside it
  const stream::Split s = stream::split(src, nbytes);
  const u32x4 *bs = reinterpret_cast<const u32x4 *>(src + s.head);
  u32x4 *bd = reinterpret_cast<u32x4 *>(dst + s.head);
  for (const stream::Chunk &c : stream::chunks(s.n16, TILE)) {
    hipLaunchKernelGGL((lut_stream_kernel<U, C3, LAYOUT>), dim3(stream::blocks(c.m, TILE, max_blocks)), dim3(kBlock), 0,
                       stream, bs + c.c0, bd + c.c0, c.m, src, dst, c.first ? s.head : 0u, src + s.tail_at(),
                       dst + s.tail_at(), c.last ? s.tail : 0u, stream::phases3(phase, s, c), tab);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_lut(const void *dsrc, void *ddst, size_t nbytes, const uint8_t *table, int channels, uint32_t phase,
                      const LaunchCfg &cfg, hipStream_t stream) {
  if (nbytes == 0) return hipSuccess;
  if (!table || (channels != 1 && channels != 3) || phase >= (uint32_t)channels) return hipErrorInvalidValue;
  LutArg tab;
  uint8_t *tb = reinterpret_cast<uint8_t *>(tab.w);
  for (int c = 0; c < 3; ++c) std::memcpy(tb + 256 * c, table + (channels == 3 ? 256 * c : 0), 256);
  const uint8_t *src = static_cast<const uint8_t *>(dsrc);
  uint8_t *dst = static_cast<uint8_t *>(ddst);
  const bool c3 = channels == 3;
  if (((uintptr_t)src ^ (uintptr_t)dst) & 15) {
    // 16 bytes per thread and grid stride at the least, so short ranges take few workgroups
    uint64_t blocks = (nbytes + (uint64_t)kBlock * 16 - 1) / ((uint64_t)kBlock * 16);
    if (blocks > (uint64_t)cfg.max_blocks) blocks = (uint64_t)cfg.max_blocks;
    if (c3) hipLaunchKernelGGL(lut_bytes_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, src, dst,
                               (uint64_t)nbytes, phase, tab);
    else hipLaunchKernelGGL(lut_bytes_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, src, dst,
                            (uint64_t)nbytes, 0u, tab);
    return hipGetLastError();
  }
  static const int layout = env_size("VF_LUT_LAYOUT", 0) == 1 ? 1 : 0;
  if (layout == 1)
    return c3 ? launch_lut_stream<true, 1>(src, dst, nbytes, phase, tab, cfg.max_blocks, stream)
              : launch_lut_stream<false, 1>(src, dst, nbytes, 0, tab, cfg.max_blocks, stream);
  return c3 ? launch_lut_stream<true, 0>(src, dst, nbytes, phase, tab, cfg.max_blocks, stream)
            : launch_lut_stream<false, 0>(src, dst, nbytes, 0, tab, cfg.max_blocks, stream);
}

}  // namespace vf
