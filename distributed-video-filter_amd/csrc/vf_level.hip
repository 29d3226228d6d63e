// vf_level.hip — the level filter on raw frames (cv2.equalizeHist, auto-levels): per
// frame a histogram of the operand, from it a 256-entry table per channel by vf_level_plan.h's
// rule, and the table applied.  Two launches per frame and no table buffer:
//
// hist_kernel streams the operand with the stream kernels' memory side (vf_stream.h: 16 B per
// lane, U = 4 loads in flight, grid-stride over whole tiles, head and tail bytes bytewise by block
// 0) and tracks a byte's channel as vf_lut.hip does (16 = 1 mod 3).  Every byte is one
// non-returning 32-bit LDS add into the workgroup's histogram; the workgroup then adds its non-zero
// bins to the frame's channels x 256 words in global memory with device-scope atomics.
//   * Same-address conflicts: flat video puts every lane of a wave on one bin.  The workgroup keeps
//     R replicas of its histogram, a lane adds to replica (lane % R), and the replicas of one bin
//     are neighbouring LDS words, so the R addresses of a flat wave fall into R banks.
//   * Counter width: every counter is 32 bits, in LDS and in global memory.  A bin counts at most
//     the frame's pixels, which the callers hold to 2^32 - 1, so none can overflow and no early
//     flush exists.
//   * Cache policy: plain loads by default; the apply pass re-reads the frame right after.
// VF_HIST_REPLICAS (1, 4, 8, 16), VF_HIST_NT (1: nontemporal loads) and VF_HIST_BLOCKS (the grid
// cap) are read once, for measurements; DESIGN.md 22.4 records what each measured.
//
// level_apply_kernel is lut_stream_kernel (vf_lut_lds.h) with the table built by the workgroup
// itself: wave c reads channel c's 256 words (with link, the masked channels' words, summed), four
// bins a lane, scans them across the wave, finds the rule's two ends by counting ballots, and
// writes level_entry of its four bins into the 768-byte LDS table.  level_bytes_kernel is the same
// for src and dst at different offsets mod 16.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "vf_env.h"
#include "vf_internal.h"
#include "vf_level_plan.h"
#include "vf_lut_lds.h"
#include "vf_stream.h"

namespace vf {

namespace {

constexpr int kHistReplicas = 8;      // LDS histograms per workgroup (24 KiB on 3 channels)
constexpr int kHistMaxBlocks = 1024;  // hist_kernel's grid cap, 4 workgroups per CU: 2048 and 8192 measured slower

__device__ __forceinline__ void lds_inc(uint32_t *p) {  // result unused: a non-returning ds_add_u32
  (void)__hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The 16 bytes of one vector counted.  h, ROT as lut16's; bin (c << 8 | v) of replica rep is word
// (c << 8 | v) * R + rep.
template <bool C3, int R, int ROT>
__device__ __forceinline__ void hist16(uint32_t *s, u32x4 v, const uint32_t h[3], uint32_t rep) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t bin = __builtin_amdgcn_perm(C3 ? h[(4 * j + k + ROT) % 3] : 0u, w[j], 0x0C0C0400u | (uint32_t)k);
      lds_inc(s + (bin * R + rep));
    }
  }
}

template <bool C3, int R, int U, int J = 0>
__device__ __forceinline__ void hist_tile(uint32_t *s, const u32x4 (&v)[U], const uint32_t h[3], uint32_t rep) {
  if constexpr (J < U) {
    hist16<C3, R, J % 3>(s, v[J], h, rep);
    hist_tile<C3, R, U, J + 1>(s, v, h, rep);
  }
}

template <bool C3, int R, bool NT, int U, int J = 0>
__device__ __forceinline__ void hist_partial(uint32_t *s, const u32x4 *src, uint64_t i0, uint64_t n16, const uint32_t h[3],
                                             uint32_t rep) {
  if constexpr (J < U) {
    const uint64_t i = i0 + (uint64_t)J * kBlock;
    if (i < n16) hist16<C3, R, J % 3>(s, ld16<NT>(src + i), h, rep);
    hist_partial<C3, R, NT, U, J + 1>(s, src, i0, n16, h, rep);
  }
}

// Body: n16 aligned 16-B vectors at src.  Head/tail: up to 15 bytes each, by block 0.  phases as
// lut_stream_kernel's.  hist: C x 256 words, added to.
template <int U, bool C3, int R, bool NT>
__global__ __launch_bounds__(kBlock) void hist_kernel(const u32x4 *__restrict__ src, uint64_t n16,
                                                      const uint8_t *__restrict__ hsrc, uint32_t head,
                                                      const uint8_t *__restrict__ tsrc, uint32_t tail, uint32_t phases,
                                                      uint32_t *__restrict__ hist) {
  constexpr int BINS = C3 ? 768 : 256;
  __shared__ uint32_t s[BINS * R];
  const uint32_t t = threadIdx.x;
  for (int i = (int)t; i < BINS * R; i += kBlock) s[i] = 0;
  __syncthreads();
  constexpr uint64_t TILE = (uint64_t)kBlock * U;
  const uint64_t stride = (uint64_t)gridDim.x * TILE;
  const uint32_t rep = t & (R - 1);
  uint64_t t0 = (uint64_t)blockIdx.x * TILE;  // wave-uniform tile start
  uint32_t c = C3 ? (uint32_t)(((phases & 3) + t0 + t) % 3) : 0;
  const uint32_t step = C3 ? (uint32_t)(stride % 3) : 0;
  for (; t0 + TILE <= n16; t0 += stride) {
    const u32x4 *sp = src + t0 + t;
    u32x4 v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) v[j] = ld16<NT>(sp + j * kBlock);
    const uint32_t h[3] = {c, mod3_inc(c, 1), mod3_inc(c, 2)};
    hist_tile<C3, R, U>(s, v, h, rep);
    c = mod3_inc(c, step);
  }
  if (t0 < n16) {  // the single partial tile, owned by whichever block reaches it
    const uint32_t h[3] = {c, mod3_inc(c, 1), mod3_inc(c, 2)};
    hist_partial<C3, R, NT, U>(s, src, t0 + t, n16, h, rep);
  }
  if (blockIdx.x == 0) {
    const uint32_t hc = C3 ? ((phases >> 2) & 3) + t : 0, tc = C3 ? ((phases >> 4) & 3) + t : 0;
    if (t < head) lds_inc(s + (((hc % 3) << 8 | hsrc[t]) * R + rep));
    if (t < tail) lds_inc(s + (((tc % 3) << 8 | tsrc[t]) * R + rep));
  }
  __syncthreads();
  for (int b = (int)t; b < BINS; b += kBlock) {
    uint32_t sum = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) sum += s[b * R + r];
    if (sum) (void)__hip_atomic_fetch_add(hist + b, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct LevelArg {
  uint32_t total;  // the entries of the histogram a table is made from: the pixels, with link times the masked channels
  int rule, mask, link, clip_lo, clip_hi;  // mask: resolved, no bit beyond the channels
};

// The workgroup's 768-byte table into s (LutLds<0>'s layout) from the frame's histogram words.
template <bool C3>
__device__ __forceinline__ void level_stage(uint32_t *s, const uint32_t *__restrict__ hist, const LevelArg &a) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave < (C3 ? 3u : 1u)) {  // wave-uniform
    uint32_t packed = 0x03020100u + 0x04040404u * lane;  // the identity of bins 4 lane .. 4 lane + 3
    if ((a.mask >> wave) & 1) {
      uint32_t h[4] = {0, 0, 0, 0};
#pragma unroll
      for (uint32_t c = 0; c < (C3 ? 3u : 1u); ++c) {
        if (a.link ? ((a.mask >> c) & 1) != 0 : c == wave) {
          const uint4 q = reinterpret_cast<const uint4 *>(hist)[c * 64 + lane];
          h[0] += q.x, h[1] += q.y, h[2] += q.z, h[3] += q.w;
        }
      }
      uint32_t cum[4];
      cum[0] = h[0], cum[1] = cum[0] + h[1], cum[2] = cum[1] + h[2], cum[3] = cum[2] + h[3];
      uint32_t incl = cum[3];  // the wave's inclusive scan of the lanes' sums
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if ((int)lane >= d) incl += up;
      }
      const uint32_t excl = incl - cum[3];
      const uint64_t total = a.total;
      const uint64_t cut_lo = a.rule == level::kStretch ? level::cut(total, a.clip_lo) : 0;
      const uint64_t cut_hi = a.rule == level::kStretch ? level::cut(total, a.clip_hi) : 0;
      // the running sums rise and the sums from the top fall, so each search counts a prefix
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cum[j] += excl;
        lo += (uint32_t)__popcll(__ballot((uint64_t)cum[j] <= cut_lo));
        hi += (uint32_t)__popcll(__ballot(total - (uint64_t)(cum[j] - h[j]) > cut_hi));
      }
      hi -= 1;  // bin 0 always counts: the cut is below half the total
      const uint32_t j_lo = lo & 3;
      const uint32_t mine = j_lo == 0 ? h[0] : j_lo == 1 ? h[1] : j_lo == 2 ? h[2] : h[3];
      const uint32_t h_lo = __shfl(mine, (int)(lo >> 2));
      const level::Scalars sc = level::level_scalars(a.rule, total, lo, hi, h_lo);
      packed = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) packed |= level::level_entry(a.rule, sc, 4 * lane + j, cum[j]) << (8 * j);
    }
    s[wave * 64 + lane] = packed;
  }
}

template <int U, bool C3>
__global__ __launch_bounds__(kBlock) void level_apply_kernel(
    const u32x4 *__restrict__ src, u32x4 *__restrict__ dst, uint64_t n16,
    const uint8_t *__restrict__ hsrc, uint8_t *__restrict__ hdst, uint32_t head,
    const uint8_t *__restrict__ tsrc, uint8_t *__restrict__ tdst, uint32_t tail, uint32_t phases,
    const uint32_t *__restrict__ hist, const LevelArg a) {
  __shared__ uint32_t s[LutLds<0>::kWords];
  level_stage<C3>(s, hist, a);
  __syncthreads();
  constexpr uint64_t TILE = (uint64_t)kBlock * U;
  const uint64_t stride = (uint64_t)gridDim.x * TILE;
  const uint32_t t = threadIdx.x;
  uint64_t t0 = (uint64_t)blockIdx.x * TILE;  // wave-uniform tile start
  uint32_t c = C3 ? (uint32_t)(((phases & 3) + t0 + t) % 3) : 0;
  const uint32_t step = C3 ? (uint32_t)(stride % 3) : 0;
  for (; t0 + TILE <= n16; t0 += stride) {
    const u32x4 *sp = src + t0 + t;
    u32x4 v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) v[j] = ld16<true>(sp + j * kBlock);
    const uint32_t h[3] = {c, mod3_inc(c, 1), mod3_inc(c, 2)};
    lut_tile<C3, 0, U>(s, v, dst + t0 + t, h);
    c = mod3_inc(c, step);
  }
  if (t0 < n16) {  // the single partial tile, owned by whichever block reaches it
    const uint32_t h[3] = {c, mod3_inc(c, 1), mod3_inc(c, 2)};
    lut_partial<C3, 0, U>(s, src, dst, t0 + t, n16, h);
  }
  if (blockIdx.x == 0) {
    const uint32_t hc = C3 ? ((phases >> 2) & 3) + t : 0, tc = C3 ? ((phases >> 4) & 3) + t : 0;
    if (t < head) hdst[t] = (uint8_t)LutLds<0>::at(s, (hc % 3) << 8 | hsrc[t]);
    if (t < tail) tdst[t] = (uint8_t)LutLds<0>::at(s, (tc % 3) << 8 | tsrc[t]);
  }
}

// src and dst at different offsets mod 16: bytewise, grid-stride, as lut_bytes_kernel.
template <bool C3>
__global__ __launch_bounds__(kBlock) void level_bytes_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                             uint64_t n, const uint32_t *__restrict__ hist,
                                                             const LevelArg a) {
  __shared__ uint32_t s[LutLds<0>::kWords];
  level_stage<C3>(s, hist, a);
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const uint32_t c = C3 ? (uint32_t)(i % 3) : 0;
    dst[i] = (uint8_t)LutLds<0>::at(s, c << 8 | src[i]);
  }
}

constexpr int kU = 4;
constexpr uint64_t kTile = (uint64_t)kBlock * kU;  // vectors per tile

template <bool C3, int R, bool NT>
hipError_t launch_hist_as(const uint8_t *src, size_t nbytes, uint32_t *hist, int max_blocks, hipStream_t stream) {
  const stream::Split s = stream::split(src, nbytes);
  const u32x4 *bs = reinterpret_cast<const u32x4 *>(src + s.head);
  for (const stream::Chunk &c : stream::chunks(s.n16, kTile)) {
    hipLaunchKernelGGL((hist_kernel<kU, C3, R, NT>), dim3(stream::blocks(c.m, kTile, max_blocks)), dim3(kBlock), 0, stream,
                       bs + c.c0, c.m, src, c.first ? s.head : 0u, src + s.tail_at(), c.last ? s.tail : 0u,
                       stream::phases3(0, s, c), hist);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <bool C3, int R>
hipError_t launch_hist_nt(const uint8_t *src, size_t nbytes, uint32_t *hist, int max_blocks, hipStream_t stream) {
  static const bool nt = env_size("VF_HIST_NT", 0) == 1;
  return nt ? launch_hist_as<C3, R, true>(src, nbytes, hist, max_blocks, stream)
            : launch_hist_as<C3, R, false>(src, nbytes, hist, max_blocks, stream);
}

template <bool C3>
hipError_t launch_hist_c(const uint8_t *src, size_t nbytes, uint32_t *hist, int max_blocks, hipStream_t stream) {
  static const size_t reps = env_size("VF_HIST_REPLICAS", kHistReplicas);
  switch (reps) {
    case 1: return launch_hist_nt<C3, 1>(src, nbytes, hist, max_blocks, stream);
    case 4: return launch_hist_nt<C3, 4>(src, nbytes, hist, max_blocks, stream);
    case 16: return launch_hist_nt<C3, 16>(src, nbytes, hist, max_blocks, stream);
    default: return launch_hist_nt<C3, kHistReplicas>(src, nbytes, hist, max_blocks, stream);
  }
}

template <bool C3>
hipError_t launch_apply(const uint8_t *src, uint8_t *dst, size_t nbytes, const uint32_t *hist, const LevelArg &a,
                        int max_blocks, hipStream_t stream) {
  if (((uintptr_t)src ^ (uintptr_t)dst) & 15) {
    uint64_t blocks = (nbytes + (uint64_t)kBlock * 16 - 1) / ((uint64_t)kBlock * 16);
    if (blocks > (uint64_t)max_blocks) blocks = (uint64_t)max_blocks;
    hipLaunchKernelGGL(level_bytes_kernel<C3>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, src, dst, (uint64_t)nbytes,
                       hist, a);
    return hipGetLastError();
  }
  const stream::Split s = stream::split(src, nbytes);
  const u32x4 *bs = reinterpret_cast<const u32x4 *>(src + s.head);
  u32x4 *bd = reinterpret_cast<u32x4 *>(dst + s.head);
  for (const stream::Chunk &c : stream::chunks(s.n16, kTile)) {
    hipLaunchKernelGGL((level_apply_kernel<kU, C3>), dim3(stream::blocks(c.m, kTile, max_blocks)), dim3(kBlock), 0, stream,
                       bs + c.c0, bd + c.c0, c.m, src, dst, c.first ? s.head : 0u, src + s.tail_at(), dst + s.tail_at(),
                       c.last ? s.tail : 0u, stream::phases3(0, s, c), hist, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_hist(const void *dsrc, size_t nbytes, int channels, uint32_t *hist, const LaunchCfg &cfg,
                       hipStream_t stream) {
  if (nbytes == 0) return hipSuccess;
  if (!dsrc || !hist || ((uintptr_t)hist & 3) || (channels != 1 && channels != 3) || nbytes % (size_t)channels != 0)
    return hipErrorInvalidValue;
  // every workgroup ends with up to channels x 256 global atomics, so the grid is capped below the
  // stream kernels' 
  static const size_t cap = env_size("VF_HIST_BLOCKS", kHistMaxBlocks);
  const int max_blocks = (int)(cap >= 1 && cap < (size_t)cfg.max_blocks ? cap : (size_t)cfg.max_blocks);
  const uint8_t *src = static_cast<const uint8_t *>(dsrc);
  return channels == 3 ? launch_hist_c<true>(src, nbytes, hist, max_blocks, stream)
                       : launch_hist_c<false>(src, nbytes, hist, max_blocks, stream);
}

hipError_t launch_level(const void *dsrc, void *ddst, size_t nbytes, int channels, int rule, int mask, int link,
                        int clip_lo, int clip_hi, uint32_t *hist, const LaunchCfg &cfg, hipStream_t stream) {
  if (nbytes == 0) return hipSuccess;
  std::string why;
  if (!dsrc || !ddst || !hist || ((uintptr_t)hist & 15) || !level::limits_ok(rule, mask, link, clip_lo, clip_hi, channels, &why) ||
      nbytes % (size_t)channels != 0 || !level::pixels_ok(nbytes / (size_t)channels, mask, link, channels, &why))
    return hipErrorInvalidValue;
  const size_t words = (size_t)channels * 256;
  hipError_t e = hipMemsetAsync(hist, 0, words * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  if ((e = launch_hist(dsrc, nbytes, channels, hist, cfg, stream)) != hipSuccess) return e;
  LevelArg a;
  a.mask = level::resolved_mask(mask, channels);
  a.total = (uint32_t)(nbytes / (size_t)channels * (size_t)(link ? level::mask_count(a.mask) : 1));
  a.rule = rule, a.link = link, a.clip_lo = clip_lo, a.clip_hi = clip_hi;
  const uint8_t *src = static_cast<const uint8_t *>(dsrc);
  uint8_t *dst = static_cast<uint8_t *>(ddst);
  return channels == 3 ? launch_apply<true>(src, dst, nbytes, hist, a, cfg.max_blocks, stream)
                       : launch_apply<false>(src, dst, nbytes, hist, a, cfg.max_blocks, stream);
}

}  // namespace vf
