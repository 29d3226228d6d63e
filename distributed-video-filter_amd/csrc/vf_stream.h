// vf_stream.h — the grid-stride streaming invert kernel and its launcher, as templates over
// the tuning parameters.  The library instantiates the one tools/tune_invert.hip measured
// fastest on MI355X (U = 4 independent 16-B loads per lane, nontemporal loads and stores:
// profiles/r01_tune_sweep{1,2,3_chunk}.txt); the tuning tool instantiates the others.
// Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vf_internal.h"
#include "vf_stream_split.h"

namespace vf {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ u32x4 ld16(const u32x4 *p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT>
__device__ __forceinline__ void st16(u32x4 *p, u32x4 v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// Body: n16 aligned 16-B vectors at src/dst.  Head/tail: up to 15 bytes each, bytewise.
// CHUNK (tools/tune_invert.hip only): block b takes the contiguous tiles [b * tpb, (b + 1) * tpb)
// instead of striding over the grid.
template <int U, bool NTL, bool NTS, bool CHUNK = false>
__global__ __launch_bounds__(kBlock) void invert_stream_kernel(
    const u32x4 *__restrict__ src, u32x4 *__restrict__ dst, uint64_t n16,
    const uint8_t *__restrict__ hsrc, uint8_t *__restrict__ hdst, uint32_t head,
    const uint8_t *__restrict__ tsrc, uint8_t *__restrict__ tdst, uint32_t tail, uint64_t tpb) {
  constexpr uint64_t TILE = (uint64_t)kBlock * U;
  const uint64_t stride = CHUNK ? TILE : (uint64_t)gridDim.x * TILE;
  const uint32_t t = threadIdx.x;
  uint64_t t0 = (uint64_t)blockIdx.x * (CHUNK ? tpb : 1) * TILE;  // wave-uniform tile start
  if (CHUNK) {
    const uint64_t e = t0 + tpb * TILE;
    n16 = e < n16 ? e : n16;
  }
  for (; t0 + TILE <= n16; t0 += stride) {
    const u32x4 *s = src + t0 + t;
    u32x4 *d = dst + t0 + t;
    u32x4 v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) v[j] = ld16<NTL>(s + j * kBlock);
#pragma unroll
    for (int j = 0; j < U; ++j) st16<NTS>(d + j * kBlock, ~v[j]);
  }
  if (t0 < n16) {  // the single partial tile, owned by whichever block reaches it
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const uint64_t i = t0 + (uint64_t)j * kBlock + t;
      if (i < n16) st16<NTS>(dst + i, ~ld16<NTL>(src + i));
    }
  }
  if (blockIdx.x == 0) {
    if (t < head) hdst[t] = (uint8_t)~hsrc[t];
    if (t < tail) tdst[t] = (uint8_t)~tsrc[t];
  }
}

// The head / body / tail split and the cut of a large body into sub-launches: vf_stream_split.h.
template <int U, bool NTL, bool NTS, bool CHUNK = false>
inline hipError_t launch_stream(const uint8_t *src, uint8_t *dst, size_t nbytes, int max_blocks,
                                hipStream_t stream) {
  constexpr uint64_t TILE = (uint64_t)kBlock * U;  // vectors per tile
  const stream::Split s = stream::split(src, nbytes);
  const u32x4 *bs = reinterpret_cast<const u32x4 *>(src + s.head);
  u32x4 *bd = reinterpret_cast<u32x4 *>(dst + s.head);
  for (const stream::Chunk &c : stream::chunks(s.n16, TILE)) {
    unsigned blocks = stream::blocks(c.m, TILE, max_blocks);
    const uint64_t tiles = (c.m + TILE - 1) / TILE;
    const uint64_t tpb = (tiles + blocks - 1) / blocks;  // CHUNK: tiles per block
    if (CHUNK && tpb) blocks = (unsigned)((tiles + tpb - 1) / tpb);
    hipLaunchKernelGGL((invert_stream_kernel<U, NTL, NTS, CHUNK>), dim3(blocks), dim3(kBlock), 0, stream, bs + c.c0,
                       bd + c.c0, c.m, src, dst, c.first ? s.head : 0u, src + s.tail_at(), dst + s.tail_at(),
                       c.last ? s.tail : 0u, tpb);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace vf
