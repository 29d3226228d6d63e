// vf_resize.hip — the resize on raw frames (cv2.resize for 8-bit frames of 1 or 3 channels: nearest,
// linear in cv2's 11-bit fixed point, area for integer shrink factors): the first
// kernels of the library whose result has another size than their operand.  vf_resize_plan.h holds
// every rule; this file holds the loops.  One launch a frame, the grid (tile x, tile y) over the
// OUTPUT, a tile kTileW pixels by `rows` rows; a lane owns one output byte column (pixel x, channel
// c) and a row's stores are consecutive bytes across the waves.
//
// resize_kernel (nearest, linear)   a lane computes its column's taps and weights once, in fp64 and
//     fp32 exactly as the plan says; the tile's row taps and weights are computed once by the first
//     lanes into LDS and read from there by everyone; everything after that is integer.  The tile's
//     source box (tile_footprint: exact, inside the frame, because every clamp is part of the rule) is
//       staged     into LDS when it fits the budget, with 16-byte loads of any alignment
//                  (tile::load16_any; the last piece of the frame's last bytes is read bytewise,
//                  nothing past the frame is touched): upscales and mild shrinks;
//       read from global memory otherwise (a strong shrink: the taps of neighbouring pixels are far
//                  apart, and most of the box is never read).
//     Linear then runs one of two forms, the same bytes either way:
//       h rows     the box is separable: the horizontally resized int32 value of every (box row,
//                  tile column) is computed once into LDS, and an output pixel is two LDS words and
//                  the vertical pass.  On an upscale several output rows share a source row, and its
//                  horizontal pass is not repeated for each of them.  Taken when the box's rows fit
//                  the h-row budget, which is 0 as committed: over a staged box it measured 5 to 9 %
//                  slower than the per-pixel form (it wins only where nothing is staged), so it
//                  stays behind its switch, for the measurement to be repeated.
//       per pixel  four taps, two horizontal passes and the vertical pass for every output pixel.
// resize_area_kernel   every source byte is read exactly once: a lane sums its block row by row
//     from global memory (a wave's loads of one block row are one contiguous span of the source row)
//     and stores the mean; no LDS.  2 x 2, the factors of cv2's linear substitution and of 4K ->
//     1080p, is a kernel of its own with the block unrolled.  A tile that touches a block overrunning
//     the frame (the fx, fy form only) goes through area_pixel's bounds instead.
// resize_area2_wide_kernel   area 2 x 2 with wide loads, taken where the source and its row pitch are
//     multiples of 4 bytes (VF_RESIZE_AREA_WIDE=0: never): a lane owns four consecutive output bytes
//     and reads what they need from both block rows as aligned dwords.
// resize_area_wide_kernel   the other factors with wide loads, under the same condition and switch: a lane
//     owns an output pixel and reads its block row's iscale_x * C consecutive bytes as aligned dwords.
// VF_RESIZE_LDS (the staged box's budget in bytes; 0: never staged), VF_RESIZE_HROWS (the h rows'
// budget in bytes; 0: per pixel everywhere), VF_RESIZE_AREA_WIDE and VF_RESIZE_ROWS (a tile's rows) are read at every
// launch, for measurements and for the tests that compare the paths in one process; DESIGN.md 26.4
// records what each measured.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "vf_env.h"
#include "vf_internal.h"
#include "vf_resize_plan.h"
#include "vf_tile.h"

namespace vf {

namespace {

constexpr int kTileW = 64;               // output pixels a tile row: a wave's lanes on 1-channel frames
constexpr int kTileRows = 16;            // output rows a tile (VF_RESIZE_ROWS; kMaxTileRows at the most)
constexpr int kMaxTileRows = 64;
constexpr uint32_t kStageLds = 16384;    // the staged box's budget in bytes (VF_RESIZE_LDS)
constexpr uint32_t kHrowLds = 0;         // the h rows' budget in bytes (VF_RESIZE_HROWS): off, it measured slower
constexpr uint32_t kMaxLds = 30720;      // of each: with the row taps below 64 KiB, no opt-in to large LDS

struct ResizeArg {
  resize::Plan p;
  int32_t rows;        // a tile's rows
  uint32_t lds, hlds;  // the two budgets, multiples of 16; 0: that form nowhere
  int32_t wide;        // area: the wide-load kernels where the source's alignment allows them
};

// Threads: the tile's byte columns times the row groups that walk its rows side by side.
template <bool C3>
struct Shape {
  static constexpr int C = C3 ? 3 : 1;
  static constexpr int kCols = kTileW * C;          // 64 or 192
  static constexpr int kGroups = C3 ? 2 : 4;
  static constexpr int kThreads = kCols * kGroups;  // 256 or 384
};

// A tap by its frame row and its byte in the row: from the frame, or from the staged box.
struct TapGlobal {
  const uint8_t *src;
  size_t row_bytes;
  __device__ __forceinline__ uint32_t operator()(int sy, int xb) const { return src[(size_t)sy * row_bytes + (size_t)xb]; }
};
struct TapLds {
  const uint8_t *staged;
  uint32_t pitch;
  int sy_lo, xb_lo;
  __device__ __forceinline__ uint32_t operator()(int sy, int xb) const {
    return staged[(uint32_t)(sy - sy_lo) * pitch + (uint32_t)(xb - xb_lo)];
  }
};

// The h rows of the lane's column for the box rows of its group.
template <class S, class Tap>
__device__ __forceinline__ void fill_hrows(int32_t *H, const Tap &tap, int col, int group, int sy_lo, int box_rows, int xb0,
                                           int xb1, int a0, int a1) {
  for (int br = group; br < box_rows; br += S::kGroups)
    H[br * S::kCols + col] = resize::linear_h((int32_t)tap(sy_lo + br, xb0), (int32_t)tap(sy_lo + br, xb1), a0, a1);
}

// The lane's pixels of its group's rows, per pixel.
template <class S, bool LINEAR, class Tap>
__device__ __forceinline__ void walk_rows(uint8_t *out, size_t out_row_bytes, const Tap &tap, const int32_t *rowc, int group,
                                          int nrows, int xb0, int xb1, int a0, int a1) {
  for (int r = group; r < nrows; r += S::kGroups) {
    const int r0 = rowc[4 * r];
    uint32_t v;
    if (LINEAR) {
      const int r1 = rowc[4 * r + 1];
      v = resize::linear_v(resize::linear_h((int32_t)tap(r0, xb0), (int32_t)tap(r0, xb1), a0, a1),
                           resize::linear_h((int32_t)tap(r1, xb0), (int32_t)tap(r1, xb1), a0, a1), rowc[4 * r + 2],
                           rowc[4 * r + 3]);
    } else {
      v = tap(r0, xb0);
    }
    out[(size_t)r * out_row_bytes] = (uint8_t)v;
  }
}

template <bool C3, bool LINEAR>
__global__ __launch_bounds__(Shape<C3>::kThreads) void resize_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                                      const ResizeArg a) {
  using S = Shape<C3>;
  constexpr int C = S::C;
  extern __shared__ __align__(16) uint8_t lds[];  // the staged box (a.lds bytes), then the h rows (a.hlds bytes)
  __shared__ int32_t rowc[4 * kMaxTileRows];      // of a tile row: the two tap rows (clamped), the two weights
  const resize::Plan &p = a.p;
  const int t = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * a.rows;
  const int x1 = (x0 + kTileW < p.dw ? x0 + kTileW : p.dw) - 1, y1 = (y0 + a.rows < p.dh ? y0 + a.rows : p.dh) - 1;
  const int nrows = y1 - y0 + 1;
  if (t < nrows) {
    if (LINEAR) {
      const resize::Coef cy = resize::row_coef(p, y0 + t);
      rowc[4 * t] = resize::clamp_index(cy.s, p.H), rowc[4 * t + 1] = resize::clamp_index(cy.s + 1, p.H);
      rowc[4 * t + 2] = cy.w0, rowc[4 * t + 3] = cy.w1;
    } else {
      rowc[4 * t] = resize::nearest_index(p.scale_y, y0 + t, p.H);
    }
  }
  // the forms: workgroup-uniform, from uniform values only
  const resize::Box b = resize::tile_footprint(p, x0, x1, y0, y1);
  const uint32_t box_bytes = (uint32_t)(b.sx_hi - b.sx_lo + 1) * C, box_rows = (uint32_t)(b.sy_hi - b.sy_lo + 1);
  const uint32_t pitch = (box_bytes + 15u) & ~15u;
  const bool staged = (uint64_t)pitch * box_rows <= (uint64_t)a.lds;
  const bool hrows = LINEAR && (uint64_t)box_rows * (S::kCols * sizeof(int32_t)) <= (uint64_t)a.hlds;
  const size_t src_row_bytes = (size_t)p.W * C;
  if (staged) {
    const uint32_t pieces = pitch >> 4, total = pieces * box_rows;
    const uint64_t frame_bytes = (uint64_t)src_row_bytes * (uint64_t)p.H;
    for (uint32_t i = (uint32_t)t; i < total; i += S::kThreads) {
      const uint32_t r = i / pieces, q = i - r * pieces;
      const uint64_t off = (uint64_t)(b.sy_lo + (int)r) * src_row_bytes + (uint64_t)b.sx_lo * C + 16u * q;
      u32x4 v;
      if (off + 16 <= frame_bytes) {
        v = tile::load16_any(src + off);
      } else {  // the frame's last bytes: nothing past them is read
        uint32_t d[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < 16 && off + j < frame_bytes; ++j) d[j >> 2] |= (uint32_t)src[off + j] << (8 * (j & 3));
        v.x = d[0], v.y = d[1], v.z = d[2], v.w = d[3];
      }
      *reinterpret_cast<u32x4 *>(lds + (size_t)r * pitch + 16u * q) = v;
    }
  }
  __syncthreads();
  const int col = t % S::kCols, group = t / S::kCols;
  const int x = x0 + col / C, c = col - (col / C) * C;
  const bool active = x <= x1;
  // the column's taps and weights: once a lane, not a row (an idle lane's are clamped into the frame too)
  int xb0, xb1 = 0, a0 = 0, a1 = 0;
  if (LINEAR) {
    const resize::Coef cx = resize::col_coef(p, x);
    xb0 = cx.s * C + c, xb1 = (cx.s + 1 < p.W ? cx.s + 1 : p.W - 1) * C + c;
    a0 = cx.w0, a1 = cx.w1;
  } else {
    xb0 = resize::nearest_index(p.scale_x, x, p.W) * C + c;
  }
  const TapGlobal tg = {src, src_row_bytes};
  const TapLds tl = {lds, pitch, b.sy_lo, b.sx_lo * C};
  const size_t out_row_bytes = (size_t)p.dw * C;
  uint8_t *out = dst + (size_t)y0 * out_row_bytes + (size_t)x * C + c;
  if (hrows) {
    int32_t *H = reinterpret_cast<int32_t *>(lds + a.lds);
    if (active) {
      if (staged)
        fill_hrows<S>(H, tl, col, group, b.sy_lo, (int)box_rows, xb0, xb1, a0, a1);
      else
        fill_hrows<S>(H, tg, col, group, b.sy_lo, (int)box_rows, xb0, xb1, a0, a1);
    }
    __syncthreads();
    if (!active) return;
    for (int r = group; r < nrows; r += S::kGroups)
      out[(size_t)r * out_row_bytes] =
          (uint8_t)resize::linear_v(H[(rowc[4 * r] - b.sy_lo) * S::kCols + col], H[(rowc[4 * r + 1] - b.sy_lo) * S::kCols + col],
                                    rowc[4 * r + 2], rowc[4 * r + 3]);
    return;
  }
  if (!active) return;
  if (staged)
    walk_rows<S, LINEAR>(out, out_row_bytes, tl, rowc, group, nrows, xb0, xb1, a0, a1);
  else
    walk_rows<S, LINEAR>(out, out_row_bytes, tg, rowc, group, nrows, xb0, xb1, a0, a1);
}

template <bool C3, bool TWO>
__global__ __launch_bounds__(Shape<C3>::kThreads) void resize_area_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                                           const ResizeArg a) {
  using S = Shape<C3>;
  constexpr int C = S::C;
  const resize::Plan &p = a.p;
  const int t = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * a.rows;
  const int x1 = (x0 + kTileW < p.dw ? x0 + kTileW : p.dw) - 1, y1 = (y0 + a.rows < p.dh ? y0 + a.rows : p.dh) - 1;
  const int col = t % S::kCols, group = t / S::kCols;
  const int x = x0 + col / C, c = col - (col / C) * C;
  if (x > x1) return;
  const int ix = TWO ? 2 : p.iscale_x, iy = TWO ? 2 : p.iscale_y;
  const size_t src_row_bytes = (size_t)p.W * C, out_row_bytes = (size_t)p.dw * C;
  uint8_t *out = dst + (size_t)x * C + c;
  // every block of the tile lies inside the frame: workgroup-uniform
  if (resize::area_whole(p, x1, y1)) {
    const uint8_t *colp = src + (size_t)x * (size_t)ix * C + c;
    for (int y = y0 + group; y <= y1; y += S::kGroups) {
      const uint8_t *rowp = colp + (size_t)y * (size_t)iy * src_row_bytes;
      uint32_t sum = 0;
      if (TWO) {
        sum = (uint32_t)rowp[0] + rowp[C] + rowp[src_row_bytes] + rowp[src_row_bytes + C];
      } else {
        for (int j = 0; j < iy; ++j, rowp += src_row_bytes)
          for (int i = 0; i < ix; ++i) sum += rowp[i * C];
      }
      out[(size_t)y * out_row_bytes] = (uint8_t)resize::area_mean(p, sum, (uint32_t)(ix * iy), true);
    }
  } else {
    for (int y = y0 + group; y <= y1; y += S::kGroups)
      out[(size_t)y * out_row_bytes] = (uint8_t)resize::area_pixel(src, p, C, c, x, y);
  }
}

// Area 2 x 2 with wide loads: a lane owns FOUR consecutive output bytes of a row and reads the source
// bytes they need -- 8 consecutive ones on 1 channel, a window of at most 12 on 3 -- from both block
// rows as aligned dwords, then sums out of registers: a quarter of the load instructions of the byte
// form, each four times as wide.  The launcher takes this kernel only when the source and its row
// pitch are multiples of 4 bytes, so an aligned dword that holds a needed byte lies inside the row
// (the row's bytes are a multiple of 4 and the needed bytes end before the row does); a dword that
// holds no needed byte is not loaded.  A lane with fewer than four valid bytes, and a tile with a
// block that overruns the frame, go through area_pixel.
template <bool C3>
__global__ __launch_bounds__(Shape<C3>::kThreads) void resize_area2_wide_kernel(const uint8_t *__restrict__ src,
                                                                                 uint8_t *__restrict__ dst, const ResizeArg a) {
  using S = Shape<C3>;
  constexpr int C = S::C;
  constexpr int kQuads = S::kCols / 4;               // lanes a tile row: 16 or 48
  constexpr int kRowGroups = S::kThreads / kQuads;   // 16 or 8
  const resize::Plan &p = a.p;
  const int t = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * a.rows;
  const int x1 = (x0 + kTileW < p.dw ? x0 + kTileW : p.dw) - 1, y1 = (y0 + a.rows < p.dh ? y0 + a.rows : p.dh) - 1;
  const int q = t % kQuads, g = t / kQuads;
  const int ob = x0 * C + 4 * q, end = (x1 + 1) * C;  // the lane's first output byte of the row; the tile's end
  if (ob >= end) return;
  const int nvalid = end - ob < 4 ? end - ob : 4;
  const size_t src_row_bytes = (size_t)p.W * C, out_row_bytes = (size_t)p.dw * C;
  const bool whole = resize::area_whole(p, x1, y1);  // workgroup-uniform
  // the source byte of output byte o, relative to the row: 2 o on 1 channel, 6 (o / 3) + o % 3 on 3
  int pos[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) pos[k] = C == 1 ? 2 * (ob + k) : 6 * ((ob + k) / 3) + (ob + k) % 3;
  const int base = pos[0] & ~3, hi = pos[3] + C;       // the window's first dword and its last needed byte
  for (int y = y0 + g; y <= y1; y += kRowGroups) {
    uint8_t *o = dst + (size_t)y * out_row_bytes + (size_t)ob;
    if (!whole || nvalid < 4) {
      for (int k = 0; k < nvalid; ++k) o[k] = (uint8_t)resize::area_pixel(src, p, C, (ob + k) % C, (ob + k) / C, y);
      continue;
    }
    const uint8_t *r0 = src + (size_t)(2 * y) * src_row_bytes + (size_t)base, *r1 = r0 + src_row_bytes;
    uint32_t d0[4] = {0, 0, 0, 0}, d1[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < (C == 1 ? 2 : 4); ++k)
      if (base + 4 * k <= hi) {
        d0[k] = *reinterpret_cast<const uint32_t *>(r0 + 4 * k);
        d1[k] = *reinterpret_cast<const uint32_t *>(r1 + 4 * k);
      }
    const uint64_t lo0 = (uint64_t)d0[0] | (uint64_t)d0[1] << 32, hi0 = (uint64_t)d0[2] | (uint64_t)d0[3] << 32;
    const uint64_t lo1 = (uint64_t)d1[0] | (uint64_t)d1[1] << 32, hi1 = (uint64_t)d1[2] | (uint64_t)d1[3] << 32;
    auto byte_at = [](uint64_t lo, uint64_t hi64, int s) -> uint32_t {
      return (uint32_t)((s < 8 ? lo >> (8 * s) : hi64 >> (8 * (s - 8))) & 255u);
    };
    uint32_t out4 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int s = pos[k] - base;  // 0 .. 11; s + C <= 14
      const uint32_t sum = byte_at(lo0, hi0, s) + byte_at(lo0, hi0, s + C) + byte_at(lo1, hi1, s) + byte_at(lo1, hi1, s + C);
      out4 |= ((sum + 2u) >> 2) << (8 * k);
    }
    if (((uintptr_t)o & 3) == 0) {
      *reinterpret_cast<uint32_t *>(o) = out4;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = (uint8_t)(out4 >> (8 * k));
    }
  }
}

// Area at any other factors with wide loads: a lane owns one output PIXEL, all its channels, whose block
// row is iscale_x * C consecutive source bytes; it reads them as the aligned dwords that hold them (at most
// 13) and adds up each channel's bytes of a dword with one sum-of-absolute-differences against 0, under a
// mask of the bytes that are inside the block row and belong to the channel (on 3 channels the channel of a
// dword's byte 0 moves on by one from a dword to the next).  A quarter of the byte form's load instructions
// or fewer.  Taken under the 2 x 2 wide kernel's condition -- the source and its row pitch are multiples of
// 4 bytes, so every such dword lies inside its row -- and a tile with a block that overruns the frame goes
// through area_pixel.
template <bool C3>
__global__ __launch_bounds__(Shape<C3>::kThreads) void resize_area_wide_kernel(const uint8_t *__restrict__ src,
                                                                                uint8_t *__restrict__ dst, const ResizeArg a) {
  using S = Shape<C3>;
  constexpr int C = S::C;
  constexpr int kRowGroups = S::kThreads / kTileW;  // 4 or 6
  const resize::Plan &p = a.p;
  const int t = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * a.rows;
  const int x1 = (x0 + kTileW < p.dw ? x0 + kTileW : p.dw) - 1, y1 = (y0 + a.rows < p.dh ? y0 + a.rows : p.dh) - 1;
  const int x = x0 + t % kTileW, g = t / kTileW;
  if (x > x1) return;
  const int ix = p.iscale_x, iy = p.iscale_y;
  const size_t src_row_bytes = (size_t)p.W * C, out_row_bytes = (size_t)p.dw * C;
  const bool whole = resize::area_whole(p, x1, y1);  // workgroup-uniform
  const int p0 = x * ix * C, pe = p0 + ix * C;       // the block row's bytes [p0, pe) of a source row
  const int base = p0 & ~3, ndw = ((pe - 1) >> 2) - (base >> 2) + 1;
  // the masks of channel 0's bytes in a dword whose byte 0 has channel 0, 1, 2: bytes 0 and 3, byte 2, byte 1
  const uint32_t kChan[3] = {0xFF0000FFu, 0x00FF0000u, 0x0000FF00u};
  for (int y = y0 + g; y <= y1; y += kRowGroups) {
    uint8_t *o = dst + (size_t)y * out_row_bytes + (size_t)x * C;
    if (!whole) {
      for (int c = 0; c < C; ++c) o[c] = (uint8_t)resize::area_pixel(src, p, C, c, x, y);
      continue;
    }
    uint32_t sum[3] = {0, 0, 0};
    const uint8_t *r = src + (size_t)y * (size_t)iy * src_row_bytes + (size_t)base;
    for (int j = 0; j < iy; ++j, r += src_row_bytes) {
      int ph = (base - p0 + 3) % 3;  // the channel of the dword's byte 0 (base - p0 is -3 .. 0)
      for (int k = 0; k < ndw; ++k) {
        const int at = base + 4 * k;  // the dword's first byte in the row
        const int lo = p0 > at ? p0 - at : 0, hi = pe - at < 4 ? pe - at : 4;  // its bytes [lo, hi) are in the block row
        const uint32_t in = (hi == 4 ? 0xFFFFFFFFu : (1u << (8 * hi)) - 1u) & ~((1u << (8 * lo)) - 1u);
        const uint32_t d = *reinterpret_cast<const uint32_t *>(r + 4 * k) & in;
        if (C == 1) {
          sum[0] = __builtin_amdgcn_sad_u8(d, 0u, sum[0]);
        } else {
          sum[0] = __builtin_amdgcn_sad_u8(d & kChan[ph], 0u, sum[0]);
          sum[1] = __builtin_amdgcn_sad_u8(d & kChan[(ph + 2) % 3], 0u, sum[1]);
          sum[2] = __builtin_amdgcn_sad_u8(d & kChan[(ph + 1) % 3], 0u, sum[2]);
          ph = (ph + 1) % 3;  // four bytes on: the channel moves on by one
        }
      }
    }
    for (int c = 0; c < C; ++c) o[c] = (uint8_t)resize::area_mean(p, sum[c], (uint32_t)(ix * iy), true);
  }
}

template <bool C3>
hipError_t launch_as(const uint8_t *src, uint8_t *dst, const ResizeArg &a, hipStream_t stream) {
  const resize::Plan &p = a.p;
  const dim3 grid((unsigned)((p.dw + kTileW - 1) / kTileW), (unsigned)((p.dh + a.rows - 1) / a.rows));
  const dim3 block(Shape<C3>::kThreads);
  if (p.mode == resize::kArea) {
    const bool aligned = ((uintptr_t)src & 3) == 0 && ((size_t)p.W * Shape<C3>::C) % 4 == 0;
    if (p.iscale_x == 2 && p.iscale_y == 2 && a.wide && aligned)
      hipLaunchKernelGGL((resize_area2_wide_kernel<C3>), grid, block, 0, stream, src, dst, a);
    else if (p.iscale_x == 2 && p.iscale_y == 2)
      hipLaunchKernelGGL((resize_area_kernel<C3, true>), grid, block, 0, stream, src, dst, a);
    else if (a.wide && aligned)
      hipLaunchKernelGGL((resize_area_wide_kernel<C3>), grid, block, 0, stream, src, dst, a);
    else
      hipLaunchKernelGGL((resize_area_kernel<C3, false>), grid, block, 0, stream, src, dst, a);
  } else if (p.mode == resize::kLinear) {
    hipLaunchKernelGGL((resize_kernel<C3, true>), grid, block, a.lds + a.hlds, stream, src, dst, a);
  } else {
    hipLaunchKernelGGL((resize_kernel<C3, false>), grid, block, a.lds, stream, src, dst, a);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_resize(const void *dsrc, void *ddst, int width, int height, int channels, int dw, int dh, double fx,
                         double fy, int interp, hipStream_t stream) {
  if (width == 0 || height == 0) return hipSuccess;
  std::string why;
  ResizeArg a;
  if (!dsrc || !ddst || width < 0 || height < 0 || !resize::limits_ok(dw, dh, fx, fy, interp, channels, &why) ||
      !resize::frame_ok((uint64_t)width, (uint64_t)height, dw, dh, fx, fy, interp, &a.p, &why))
    return hipErrorInvalidValue;
  const size_t lds = env_size("VF_RESIZE_LDS", kStageLds), hlds = env_size("VF_RESIZE_HROWS", kHrowLds),
               rows = env_size("VF_RESIZE_ROWS", kTileRows);
  a.lds = (uint32_t)(lds > kMaxLds ? kMaxLds : lds) & ~15u;
  a.hlds = (uint32_t)(hlds > kMaxLds ? kMaxLds : hlds) & ~15u;
  a.wide = env_size("VF_RESIZE_AREA_WIDE", 1) != 0;
  a.rows = (int32_t)(rows < 1 ? 1 : rows > (size_t)kMaxTileRows ? (size_t)kMaxTileRows : rows);
  if ((a.p.dh + a.rows - 1) / a.rows > 65535) a.rows = kMaxTileRows;  // never: a side is at most 32767
  const uint8_t *src = static_cast<const uint8_t *>(dsrc);
  uint8_t *dst = static_cast<uint8_t *>(ddst);
  return channels == 3 ? launch_as<true>(src, dst, a, stream) : launch_as<false>(src, dst, a, stream);
}

}  // namespace vf
