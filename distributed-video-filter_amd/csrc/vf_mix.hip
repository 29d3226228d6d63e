// vf_mix.hip — the colour-matrix kernel (cv2.transform on uint8 BGR pixels):
//   acc[c] = sum_k M[c][k] * src[k] + t[c],  dst[c] = clamp(round(acc[c] / 2^shift), 0, 255)
// per 3-byte pixel, c, k in {0, 1, 2}, the rounding half to even or (acc + half) >> shift.
// Pointwise like the table and binary kernels, but its element is a whole pixel inside the 16-B
// per lane stream, and it has real arithmetic.
//
// The memory side is vf_binary.hip's: nontemporal 16-B accesses, the 16-B grid is dst's (every body
// store one aligned nontemporal 16-B store), src at another alignment read through load16_any,
// grid-stride over whole tiles, head and tail done by block 0.
//   * The pixel grid.  A lane's unit is 48 B: 16 pixels, three vectors, 12 dwords, in which the
//     pattern "4 pixels in 3 dwords" repeats four times.  The body starts where a pixel starts and
//     where dst is 16-B aligned (vf_pixel_split.h: a head of at most 15 pixels always exists); the
//     tail is under 48 B.  Block 0 does both pixel by pixel.  A tile is kBlock * U units.
//   * Two forms of the body.  In the stride form a lane takes its own units, so the lanes of a wave
//     sit 48 B apart and each of the wave's loads touches 3 KiB for 1 KiB of data: measured, it runs
//     at 1.67 x the table kernel's time whatever the rounding (profiles/mix_raw_bench.txt).  In the
//     coalesced form, the default for whole tiles, a wave takes a chunk of 3 KiB (1024 pixels) and
//     lane l the vectors l, l + 64 and l + 128, so every access covers 1 KiB without a gap; the one
//     or two bytes of a pixel that straddles two vectors come from the neighbour lane through
//     ds_bpermute_b32, and such a pixel is computed by both lanes (6 pixels per vector for 5 1/3):
//     1.05 - 1.09 x the table kernel.  The partial tile takes the stride form; VF_MIX_FORM=stride
//     gives every tile to it (tools/mix_bench.py, tests).
//   * A pixel is read and written by the same lane, the reads first, so dst == src exactly is
//     allowed; partial overlap is the caller's to refuse (vf_mix_device does).
//   * The arithmetic.  Weights fit int16 and inputs are 0 .. 255, so an output channel is two
//     v_dot2_i32_i16 (__builtin_amdgcn_sdot2) on the pairs (b, g) and (r, 0), the accumulator
//     starting at t[c] (plus 2^(shift - 1) for half_up).  With sum_k |M[c][k]| <= 65536 and
//     |t[c]| <= 255 * 2^shift <= 255 * 65536:  |acc| <= 255 * 65536 + 255 * 65536 < 2^25, and with
//     the rounding addend |acc + 2^(shift - 1)| < 2^25 + 2^15: far inside int32, no dot saturates.
//     The pairs are unpacked with v_perm_b32, the sum is clamped by min / max against 0 and
//     (256 << shift) - 1 (one v_med3_i32) before the shift, and packed back with shift-or.  The kernel is instantiated per rounding
//     (none for shift 0, half_up, half_even), so the half-even correction costs nothing elsewhere.
// Nothing is written outside [dst, dst + nbytes).  No device allocation; the launch stays
// asynchronous on the caller's stream.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <cstdlib>
#include <cstring>

#include "vf_internal.h"
#include "vf_pixel_split.h"
#include "vf_stream.h"
#include "vf_tile.h"

namespace vf {

namespace {

using tile::load16_any;

typedef short s2 __attribute__((ext_vector_type(2)));

enum : int { kNone = 0, kHalfUp = 1, kHalfEven = 2 };  // the kernel's rounding forms

constexpr int kUnits = 2;  // units of 48 B per lane per tile: 6 vectors in flight

struct MixArgs {
  uint32_t wbg[3];  // M[c][0] in the low half, M[c][1] in the high half (two int16)
  uint32_t wr[3];   // M[c][2] in the low half, 0 above
  int32_t init[3];  // t[c], plus 2^(shift - 1) for half_up
  int32_t shift;
  int32_t hm1;      // half_even: 2^(shift - 1) - 1
  int32_t top;      // (256 << shift) - 1: the largest sum that still gives 255
};

// One output channel of a pixel given as (b, g) and (r, 0) in 16-bit halves.
template <int R>
__device__ __forceinline__ uint32_t mix1(uint32_t bg, uint32_t r0, int c, const MixArgs &m) {
  int acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(s2, r0), __builtin_bit_cast(s2, m.wr[c]), m.init[c], false);
  acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(s2, bg), __builtin_bit_cast(s2, m.wbg[c]), acc, false);
  // half_up: the half is in init.  half_even: + (h - 1) + (f odd) carries into the quotient when
  // r > h, or r == h and f is odd.
  if constexpr (R == kHalfEven) acc += m.hm1 + ((acc >> m.shift) & 1);
  // The clamp comes BEFORE the shift: min(max(x >> s, 0), 255) == min(max(x, 0), (256 << s) - 1) >> s
  // for the flooring shift, one v_med3_i32 and one logical shift.  Written as shift-then-clamp the
  // compiler fuses shift, clamp and the pack of two results into v_ashr_pk_u8_i32 and ORs the
  // other two bytes of the dword on top of it; on the MI355X those two bytes then came out 255
  // wherever the packed sums were negative.
  // top is not a compile-time constant, so min / max would stay two instructions: the median is
  // written out (top >= 0 always: med3(acc, 0, top) is the clamp)
  asm("v_med3_i32 %0, %1, 0, %2" : "=v"(acc) : "v"(acc), "s"(m.top));
  if constexpr (R == kNone) return (uint32_t)acc;
  else return (uint32_t)acc >> m.shift;
}

// Four pixels in the three dwords w0, w1, w2 (bytes b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3).
template <int R>
__device__ __forceinline__ void mix4(uint32_t &w0, uint32_t &w1, uint32_t &w2, const MixArgs &m) {
  const uint32_t bg[4] = {__builtin_amdgcn_perm(0u, w0, 0x0C010C00u), __builtin_amdgcn_perm(w1, w0, 0x0C040C03u),
                          __builtin_amdgcn_perm(0u, w1, 0x0C030C02u), __builtin_amdgcn_perm(0u, w2, 0x0C020C01u)};
  const uint32_t r0[4] = {__builtin_amdgcn_perm(0u, w0, 0x0C0C0C02u), __builtin_amdgcn_perm(0u, w1, 0x0C0C0C01u),
                          __builtin_amdgcn_perm(0u, w2, 0x0C0C0C00u), __builtin_amdgcn_perm(0u, w2, 0x0C0C0C03u)};
  uint32_t o[12];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int c = 0; c < 3; ++c) o[3 * p + c] = mix1<R>(bg[p], r0[p], c, m);
  w0 = (o[0] | o[1] << 8) | (o[2] | o[3] << 8) << 16;
  w1 = (o[4] | o[5] << 8) | (o[6] | o[7] << 8) << 16;
  w2 = (o[8] | o[9] << 8) | (o[10] | o[11] << 8) << 16;
}

// One unit: 16 pixels in three vectors.
template <int R>
__device__ __forceinline__ void mix_unit(u32x4 &v0, u32x4 &v1, u32x4 &v2, const MixArgs &m) {
  uint32_t w[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
#pragma unroll
  for (int g = 0; g < 4; ++g) mix4<R>(w[3 * g], w[3 * g + 1], w[3 * g + 2], m);
  v0 = u32x4{w[0], w[1], w[2], w[3]};
  v1 = u32x4{w[4], w[5], w[6], w[7]};
  v2 = u32x4{w[8], w[9], w[10], w[11]};
}

// Two pixels in w0 and the low half of w1 (bytes b0 g0 r0 b1 | g1 r1 . .).
template <int R>
__device__ __forceinline__ void mix2(uint32_t &w0, uint32_t &w1, const MixArgs &m) {
  const uint32_t bg[2] = {__builtin_amdgcn_perm(0u, w0, 0x0C010C00u), __builtin_amdgcn_perm(w1, w0, 0x0C040C03u)};
  const uint32_t r0[2] = {__builtin_amdgcn_perm(0u, w0, 0x0C0C0C02u), __builtin_amdgcn_perm(0u, w1, 0x0C0C0C01u)};
  uint32_t o[6];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int c = 0; c < 3; ++c) o[3 * p + c] = mix1<R>(bg[p], r0[p], c, m);
  w0 = (o[0] | o[1] << 8) | (o[2] | o[3] << 8) << 16;
  w1 = o[4] | o[5] << 8;
}

// The coalesced form's step: one 16-B vector whose byte 0 is byte `ph` (0 .. 2) of a pixel, with the
// dword before it (`prev`, from the lane below) and the dword after it (`next`, from the lane
// above).  The six pixels that touch the vector start at byte 4 - ph of the 24-byte window
// prev | v | next; they are shifted down to byte 0 (two v_alignbyte_b32 per dword, the second with
// the lane's own count), mixed at fixed positions, and the vector's 16 result bytes are shifted
// back out.  A pixel that straddles two vectors is computed by both lanes; each keeps its bytes.
template <int R>
__device__ __forceinline__ u32x4 mix_vector(uint32_t prev, u32x4 v, uint32_t next, uint32_t ph, const MixArgs &m) {
  const uint32_t w[6] = {prev, v.x, v.y, v.z, v.w, next};
  uint32_t u[6], r[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) u[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], 2u);  // window bytes 2 .. 21
  u[5] = 0u;
#pragma unroll
  for (int k = 0; k < 5; ++k) r[k] = __builtin_amdgcn_alignbyte(u[k + 1], u[k], 2u - ph);  // from byte 4 - ph
  mix4<R>(r[0], r[1], r[2], m);
  mix2<R>(r[3], r[4], m);
  u32x4 o;  // result byte i of r is window byte 4 - ph + i: the vector's are bytes ph .. ph + 15
  o.x = __builtin_amdgcn_alignbyte(r[1], r[0], ph);
  o.y = __builtin_amdgcn_alignbyte(r[2], r[1], ph);
  o.z = __builtin_amdgcn_alignbyte(r[3], r[2], ph);
  o.w = __builtin_amdgcn_alignbyte(r[4], r[3], ph);
  return o;
}

// One wave's chunk of the coalesced form: 192 vectors = 3 KiB = 1024 whole pixels; lane l holds the
// vectors l, l + 64 and l + 128, so each of the wave's three loads and stores covers 1 KiB without a
// gap.  Vector n starts at byte n % 3 of a pixel (16 = 1 mod 3).  The neighbours' dwords come through
// ds_bpermute_b32 (the LDS crossbar; no LDS is allocated): lane 0's "before" is lane 63's of the
// row before, lane 63's "after" is lane 0's of the row after, and the chunk's two ends are pixel
// boundaries, where nothing is needed.
template <int R>
__device__ __forceinline__ void mix_chunk(u32x4 (&x)[3], uint32_t lane, const MixArgs &m) {
  const int below = (int)(((lane + 63u) & 63u) << 2), above = (int)(((lane + 1u) & 63u) << 2);
  uint32_t up[3], dn[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    up[j] = (uint32_t)__builtin_amdgcn_ds_bpermute(below, (int)x[j].w);  // lane 0 gets lane 63's
    dn[j] = (uint32_t)__builtin_amdgcn_ds_bpermute(above, (int)x[j].x);  // lane 63 gets lane 0's
  }
  const uint32_t l3 = lane % 3u;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const uint32_t prev = lane == 0 ? (j == 0 ? 0u : up[j == 0 ? 0 : j - 1]) : up[j];
    const uint32_t next = lane == 63 ? (j == 2 ? 0u : dn[j == 2 ? 2 : j + 1]) : dn[j];
    uint32_t ph = l3 + (uint32_t)j;  // (lane + 64 j) % 3
    ph = ph >= 3u ? ph - 3u : ph;
    x[j] = mix_vector<R>(prev, x[j], next, ph, m);
  }
}

template <int R>
__device__ __forceinline__ void mix_pixel(const uint8_t *s, uint8_t *d, const MixArgs &m) {
  const uint32_t bg = (uint32_t)s[0] | (uint32_t)s[1] << 16, r0 = s[2];  // the reads first: d may be s
  const uint32_t b = mix1<R>(bg, r0, 0, m), g = mix1<R>(bg, r0, 1, m), r = mix1<R>(bg, r0, 2, m);
  d[0] = (uint8_t)b;
  d[1] = (uint8_t)g;
  d[2] = (uint8_t)r;
}

// Body: `units` units of 48 B at src / dst, dst 16-B aligned, src at any alignment.
// Head / tail: up to 15 pixels each, pixel by pixel by block 0.
// COAL: whole tiles in the coalesced form (a tile is 4 waves x U chunks of 64 units), else every lane
// its own units at a stride of 48 B; the partial tile takes the stride form in both.
template <int R, int U, bool COAL>
__global__ __launch_bounds__(kBlock) void mix_kernel(const uint8_t *src, u32x4 *dst, uint64_t units, MixArgs m,
                                                     const uint8_t *hsrc, uint8_t *hdst, uint32_t head_px,
                                                     const uint8_t *tsrc, uint8_t *tdst, uint32_t tail_px) {
  constexpr uint64_t TILE = (uint64_t)kBlock * U;  // units per tile
  const uint64_t stride = (uint64_t)gridDim.x * TILE;
  const uint32_t t = threadIdx.x;
  uint64_t t0 = (uint64_t)blockIdx.x * TILE;  // wave-uniform tile start
  if constexpr (COAL) {
    const uint32_t lane = t & 63u, wave = t >> 6;
    for (; t0 + TILE <= units; t0 += stride) {
      u32x4 x[U][3];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const uint8_t *p = src + (t0 + ((uint64_t)j * (kBlock / 64) + wave) * 64) * pixel::kUnitBytes + 16 * lane;
#pragma unroll
        for (int k = 0; k < 3; ++k) x[j][k] = load16_any(p + 1024 * k);
      }
#pragma unroll
      for (int j = 0; j < U; ++j) {
        mix_chunk<R>(x[j], lane, m);
        u32x4 *d = dst + (t0 + ((uint64_t)j * (kBlock / 64) + wave) * 64) * 3 + lane;
#pragma unroll
        for (int k = 0; k < 3; ++k) st16<true>(d + 64 * k, x[j][k]);
      }
    }
  }
  for (; t0 + TILE <= units; t0 += stride) {
    u32x4 x[U][3];
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const uint8_t *p = src + (t0 + (uint64_t)j * kBlock + t) * pixel::kUnitBytes;
#pragma unroll
      for (int k = 0; k < 3; ++k) x[j][k] = load16_any(p + 16 * k);
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      mix_unit<R>(x[j][0], x[j][1], x[j][2], m);
      u32x4 *d = dst + (t0 + (uint64_t)j * kBlock + t) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) st16<true>(d + k, x[j][k]);
    }
  }
  if (t0 < units) {  // the single partial tile, owned by whichever block reaches it
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const uint64_t i = t0 + (uint64_t)j * kBlock + t;
      if (i < units) {
        const uint8_t *p = src + i * pixel::kUnitBytes;
        u32x4 v0 = load16_any(p), v1 = load16_any(p + 16), v2 = load16_any(p + 32);
        mix_unit<R>(v0, v1, v2, m);
        st16<true>(dst + i * 3, v0);
        st16<true>(dst + i * 3 + 1, v1);
        st16<true>(dst + i * 3 + 2, v2);
      }
    }
  }
  if (blockIdx.x == 0) {
    if (t < head_px) mix_pixel<R>(hsrc + 3 * t, hdst + 3 * t, m);
    if (t < tail_px) mix_pixel<R>(tsrc + 3 * t, tdst + 3 * t, m);
  }
}

template <int R, bool COAL>
hipError_t launch_form(const uint8_t *src, uint8_t *dst, size_t nbytes, const MixArgs &m, int max_blocks,
                       hipStream_t stream) {
  const pixel::Split s = pixel::split(dst, nbytes);  // the 16-B grid is dst's
  const size_t t = s.tail_at();
  hipLaunchKernelGGL((mix_kernel<R, kUnits, COAL>), dim3(stream::blocks(s.units, (uint64_t)kBlock * kUnits, max_blocks)),
                     dim3(kBlock), 0, stream, src + s.head, reinterpret_cast<u32x4 *>(dst + s.head), s.units, m, src, dst,
                     s.head / 3, src + t, dst + t, s.tail / 3);
  return hipGetLastError();
}

}  // namespace

size_t mix_tile_bytes() { return (size_t)kBlock * kUnits * pixel::kUnitBytes; }

hipError_t launch_mix(const void *dsrc, void *ddst, size_t nbytes, const int32_t m[12], int shift, int rounding,
                      const LaunchCfg &cfg, hipStream_t stream) {
  if (nbytes == 0) return hipSuccess;
  if (!dsrc || !ddst || !m || nbytes % 3 != 0 || shift < 0 || shift > 16 || (rounding != 0 && rounding != 1) ||
      cfg.max_blocks < 1)
    return hipErrorInvalidValue;
  MixArgs a;
  for (int c = 0; c < 3; ++c) {
    a.wbg[c] = ((uint32_t)m[4 * c] & 0xFFFFu) | ((uint32_t)m[4 * c + 1] & 0xFFFFu) << 16;
    a.wr[c] = (uint32_t)m[4 * c + 2] & 0xFFFFu;
    a.init[c] = m[4 * c + 3] + (shift > 0 && rounding == 1 ? 1 << (shift - 1) : 0);
  }
  a.shift = shift;
  a.hm1 = shift > 0 ? (1 << (shift - 1)) - 1 : 0;
  a.top = (256 << shift) - 1;
  const uint8_t *src = static_cast<const uint8_t *>(dsrc);
  uint8_t *dst = static_cast<uint8_t *>(ddst);
  const char *e = std::getenv("VF_MIX_FORM");  // read per call: tools/mix_bench.py switches it in-process
  if (e && std::strcmp(e, "stride") == 0) {
    if (shift == 0) return launch_form<kNone, false>(src, dst, nbytes, a, cfg.max_blocks, stream);
    if (rounding == 1) return launch_form<kHalfUp, false>(src, dst, nbytes, a, cfg.max_blocks, stream);
    return launch_form<kHalfEven, false>(src, dst, nbytes, a, cfg.max_blocks, stream);
  }
  if (shift == 0) return launch_form<kNone, true>(src, dst, nbytes, a, cfg.max_blocks, stream);
  if (rounding == 1) return launch_form<kHalfUp, true>(src, dst, nbytes, a, cfg.max_blocks, stream);
  return launch_form<kHalfEven, true>(src, dst, nbytes, a, cfg.max_blocks, stream);
}

}  // namespace vf
