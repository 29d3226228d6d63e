// vf_sep.hip — the separable filter on raw frames: cv2.sepFilter2D(frame, -1, kx / 2^sx, ky / 2^sy),
// cv2.blur and cv2.boxFilter for uint8 frames of 1 or 3 interleaved channels, integer taps, odd tap
// counts up to 31 per axis, exact (DESIGN.md 21 has the definition).
//
// A frame is H rows of W * C bytes and the horizontal neighbour of a byte is C bytes away, so the
// kernel works on bytes and never de-interleaves, as vf_conv.hip.  A workgroup (256 lanes) owns a
// tile of g.rows rows x 256 row bytes (vf_sep_plan.h has the geometry) and goes through it in
// four steps with a barrier between them, all in LDS:
//   * staging: the tile with its halo, (rows + 2 ry) rows x stage_bytes bytes, in 16-B pieces with
//     the borders resolved in frame coordinates (vf_conv_border.h): a piece that leaves the row is
//     put together byte by byte, so the passes have no border branches;
//   * vertical pass: one lane per dword of a row, kh taps down the staged rows, into rows x
//     stage_bytes wide sums: int16 when 255 * sum|ky| < 2^15, else int32.  Nothing is rounded;
//   * horizontal pass: one wave per row, lane l makes bytes l, l + 64, l + 128 and l + 192 of it, so
//     every LDS read of a wave is 64 adjacent sums; kw taps, the one rounding (a shift or the exact
//     division of vf_sep_plan.h), the clamp, and the byte goes into LDS over the staged bytes;
//   * store: 16 B per lane, nontemporal when the address is 16-B aligned, else dwords or bytes.
// Both LDS pitches are stage_bytes without padding: in the staging and in both passes adjacent lanes
// touch adjacent elements, so every access is conflict free whatever the pitch.
// The taps, the scale and the geometry are by-value kernel arguments: no device allocation, and the
// launch stays asynchronous on the caller's stream.  One instantiation per channel count and sum
// width; the tap counts and the geometry are not compile-time values.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <cstdlib>
#include <cstring>

#include "vf_conv_border.h"
#include "vf_internal.h"
#include "vf_sep_plan.h"
#include "vf_stream.h"
#include "vf_tile.h"

namespace vf {

namespace {

using tile::load16_any;
using tile::Rows;

struct SepArgs {
  Rows r;
  int32_t kw, kh;
  int32_t rxc;                       // (kw / 2) * C: the bytes a horizontal tap reaches
  int32_t rows, halo, stage_rows;    // sep::Geometry
  int32_t stage_bytes;
  uint32_t pieces_recip;             // sep::recip of stage_bytes / 16
  int32_t shift, add, odd, top;      // the shift's rounding: (acc + add + ((acc >> shift) & odd)) clamped to top, >> shift
  int32_t d, dtop;                   // sep::Divide; d == 1: the shift form
  uint64_t dmul;
  int32_t kx[sep::kMaxSide], ky[sep::kMaxSide];  // int16 values, a dword each: a tap is one scalar load
};

__device__ __forceinline__ uint32_t finish(int acc, const SepArgs &a) {
  if (a.d > 1) {
    // the clamp first: 2 acc + d < 2^20, and the product fits 64 bits
    const int c = min(max(acc, 0), a.dtop);
    return (uint32_t)(((uint64_t)(uint32_t)(2 * c + a.d) * a.dmul) >> 40);
  }
  // half_up: add is the half.  half_even: add = half - 1, + 1 when floor(acc / 2^shift) is odd.
  // The clamp comes BEFORE the shift: min(max(x >> s, 0), 255) ==
  // min(max(x, 0), (256 << s) - 1) >> s for the flooring shift.
  acc += a.add + ((acc >> a.shift) & a.odd);
  acc = min(max(acc, 0), a.top);
  return (uint32_t)acc >> a.shift;
}

template <int C, bool NARROW>
__global__ __launch_bounds__(kBlock) void sep_kernel(const SepArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  using Mid = typename std::conditional<NARROW, int16_t, int32_t>::type;
  const int SB = a.stage_bytes;
  uint8_t *stage = lds;                                             // stage_rows x SB bytes
  Mid *mid = reinterpret_cast<Mid *>(lds + a.stage_rows * SB);      // rows x SB sums (SB % 16 == 0)
  const int tid = (int)threadIdx.x;
  const int ry = a.kh >> 1;
  const int64_t tile_x = (int64_t)blockIdx.x * sep::kTileBytes;  // row offset of the tile's first byte
  const int ty0 = a.r.y0 + (int)blockIdx.y * a.rows;             // frame row of the tile's first row
  const int yend = a.r.y0 + a.r.nrows;
  const int live = min(a.rows, yend - ty0);                      // the tile's rows inside the launch

  // ---- stage the tile and its halo, borders resolved ------------------------------------------
  const int pieces = SB >> 4;
  for (int item = tid; item < a.stage_rows * pieces; item += kBlock) {
    const int r = (int)__umulhi((uint32_t)item, a.pieces_recip), c = item - r * pieces;
    const int fy_raw = ty0 - ry + r;
    u32x4 v;
    v.x = v.y = v.z = v.w = 0;
    if (fy_raw < yend + ry) {  // rows below the last output row's halo are never read
      const int fy = conv::border_index(fy_raw, a.r.h, a.r.border);
      const int sr = fy - a.r.s0;
      if (fy >= 0 && sr >= 0 && sr < a.r.nsrc) {
        const uint8_t *row = a.r.src + (size_t)sr * a.r.row_bytes;
        const int64_t o = tile_x - a.halo + 16 * c;  // row offset of the piece
        if (o >= 0 && o + 16 <= (int64_t)a.r.row_bytes) {
          v = load16_any(row + o);
        } else {
          uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const int64_t off = o + k;
            // floor(off / C) for off >= -48 (the largest halo)
            const int64_t px = (off + (int64_t)48 * C) / C - 48;
            uint32_t val = 0;
            if (off >= -(int64_t)a.rxc && off < (int64_t)a.r.row_bytes + a.rxc) {  // only bytes a tap of the frame can reach
              const int ch = (int)(off - px * C);
              const int bx = conv::border_index((int)px, a.r.w, a.r.border);
              if (bx >= 0) val = row[(size_t)bx * C + ch];
            }
            d[k >> 2] |= val << (8 * (k & 3));
          }
          v.x = d[0];
          v.y = d[1];
          v.z = d[2];
          v.w = d[3];
        }
      }
    }
    *reinterpret_cast<u32x4 *>(stage + item * 16) = v;  // r * SB + 16 * c == 16 * item
  }
  __syncthreads();

  // ---- vertical pass: 4 adjacent sums per item ---------------------------------------------------
  const int dwords = SB >> 2;
  const uint32_t *sw = reinterpret_cast<const uint32_t *>(stage);
  for (int item = tid; item < live * dwords; item += kBlock) {
    int acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
    const uint32_t *p = sw + item;  // staged row r + j, dword g: (r + j) * dwords + g == item + j * dwords
    for (int j = 0; j < a.kh; ++j) {
      const uint32_t w = p[j * dwords];
      const int k = a.ky[j];
      acc0 += k * (int)(w & 0xFFu);
      acc1 += k * (int)((w >> 8) & 0xFFu);
      acc2 += k * (int)((w >> 16) & 0xFFu);
      acc3 += k * (int)(w >> 24);
    }
    if constexpr (NARROW) {
      uint2 o;
      o.x = ((uint32_t)acc0 & 0xFFFFu) | (uint32_t)acc1 << 16;
      o.y = ((uint32_t)acc2 & 0xFFFFu) | (uint32_t)acc3 << 16;
      reinterpret_cast<uint2 *>(mid)[item] = o;
    } else {
      int4 o;
      o.x = acc0, o.y = acc1, o.z = acc2, o.w = acc3;
      reinterpret_cast<int4 *>(mid)[item] = o;
    }
  }
  __syncthreads();

  // ---- horizontal pass: a wave per row, the results as bytes over the staged bytes ------------------
  const int lane = tid & 63;
  uint8_t *res = stage;  // rows x 256 bytes <= stage_rows x SB
  for (int r = tid >> 6; r < live; r += kBlock / 64) {
    const Mid *p = mid + r * SB + a.halo - a.rxc + lane;
    int acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
    for (int i = 0; i < a.kw; ++i) {
      const int k = a.kx[i];
      const Mid *q = p + i * C;
      acc0 += k * (int)q[0];
      acc1 += k * (int)q[64];
      acc2 += k * (int)q[128];
      acc3 += k * (int)q[192];
    }
    uint8_t *o = res + r * sep::kTileBytes + lane;
    o[0] = (uint8_t)finish(acc0, a);
    o[64] = (uint8_t)finish(acc1, a);
    o[128] = (uint8_t)finish(acc2, a);
    o[192] = (uint8_t)finish(acc3, a);
  }
  __syncthreads();

  // ---- store: inside the row and inside the launch's rows only ------------------------------------
  const int lx = tid & 15;
  const int64_t o = tile_x + 16 * lx;
  if (o >= (int64_t)a.r.row_bytes) return;
  const int64_t left = (int64_t)a.r.row_bytes - o;
  for (int r = tid >> 4; r < live; r += kBlock / 16) {
    const u32x4 v = *reinterpret_cast<const u32x4 *>(res + r * sep::kTileBytes + 16 * lx);
    uint8_t *dp = a.r.dst + (size_t)(ty0 + r - a.r.y0) * a.r.row_bytes + o;
    if (left >= 16 && ((uintptr_t)dp & 15) == 0) {
      st16<true>(reinterpret_cast<u32x4 *>(dp), v);
    } else if (left >= 16 && ((uintptr_t)dp & 3) == 0) {
      uint32_t *p4 = reinterpret_cast<uint32_t *>(dp);
      p4[0] = v.x;
      p4[1] = v.y;
      p4[2] = v.z;
      p4[3] = v.w;
    } else {
      const uint32_t d[4] = {v.x, v.y, v.z, v.w};
      const int n = left < 16 ? (int)left : 16;
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < n) dp[k] = (uint8_t)(d[k >> 2] >> (8 * (k & 3)));
    }
  }
}

template <int C>
hipError_t launch_c(const SepArgs &a, bool narrow, dim3 grid, unsigned lds, hipStream_t stream) {
  if (narrow) hipLaunchKernelGGL((sep_kernel<C, true>), grid, dim3(kBlock), lds, stream, a);
  else hipLaunchKernelGGL((sep_kernel<C, false>), grid, dim3(kBlock), lds, stream, a);
  return hipGetLastError();
}

}  // namespace

int sep_form_env() {
  const char *e = std::getenv("VF_SEP_FORM");  // read per call: tests and tools switch it in-process
  return e && std::strcmp(e, "wide") == 0 ? 1 : 0;
}

int sep_tile_rows(int kh) {
  const char *e = std::getenv("VF_SEP_ROWS");  // a measurement's override: 16, 24 or 32 where the LDS allows
  const int rows = e ? std::atoi(e) : 0;
  if (sep::rows_ok(rows) && sep::geometry(sep::kMaxSide, kh, 3, false, rows).lds_bytes <= sep::kMaxLds) return rows;
  return sep::tile_rows(kh);
}

hipError_t launch_sep(const void *dsrc, void *ddst, int width, int channels, int frame_h, int y0, int nrows, int s0,
                      int nsrc, const int16_t *kx, int kw, const int16_t *ky, int kh, int shift, int divisor,
                      int rounding, int border, int form, hipStream_t stream) {
  if (nrows <= 0 || width <= 0) return hipSuccess;
  if (!tile::rows_ok(dsrc, ddst, width, channels, frame_h, y0, nrows, s0, nsrc) ||
      !sep::limits_ok(kx, kw, ky, kh, shift, divisor, rounding, border, nullptr))
    return hipErrorInvalidValue;
  const bool narrow = form != 1 && sep::narrow_fits(ky, kh);
  const sep::Geometry g = sep::geometry(kw, kh, channels, narrow, sep_tile_rows(kh));
  if (g.lds_bytes > sep::kMaxLds) return hipErrorInvalidValue;
  SepArgs a;
  std::memset(&a, 0, sizeof a);
  a.kw = kw, a.kh = kh;
  a.rxc = (kw / 2) * channels;
  a.rows = g.rows, a.halo = g.halo, a.stage_rows = g.stage_rows, a.stage_bytes = g.stage_bytes;
  a.pieces_recip = sep::recip((uint32_t)g.stage_bytes / 16);
  a.shift = shift;
  a.add = shift == 0 ? 0 : rounding == sep::kRoundHalfUp ? 1 << (shift - 1) : (1 << (shift - 1)) - 1;
  a.odd = shift != 0 && rounding == sep::kRoundHalfEven ? 1 : 0;
  a.top = (256 << shift) - 1;
  const sep::Divide dv = sep::divide_by(divisor);
  a.d = dv.d, a.dtop = dv.top, a.dmul = dv.mul;
  for (int i = 0; i < kw; ++i) a.kx[i] = kx[i];
  for (int j = 0; j < kh; ++j) a.ky[j] = ky[j];
  Rows *r = &a.r;
  r->src = static_cast<const uint8_t *>(dsrc);
  r->row_bytes = (uint32_t)width * (uint32_t)channels;
  r->w = width;
  r->h = frame_h;
  r->s0 = s0;
  r->nsrc = nsrc;
  r->border = border;
  const unsigned gx = (r->row_bytes + sep::kTileBytes - 1) / sep::kTileBytes;
  for (const tile::RowChunk &c : tile::row_chunks(nrows)) {  // the grid's y limit: tiles are 16 rows or more
    r->y0 = y0 + c.done;
    r->nrows = c.m;
    r->dst = static_cast<uint8_t *>(ddst) + (size_t)c.done * r->row_bytes;
    const dim3 grid(gx, (unsigned)((c.m + g.rows - 1) / g.rows));
    const hipError_t e = channels == 3 ? launch_c<3>(a, narrow, grid, (unsigned)g.lds_bytes, stream)
                                       : launch_c<1>(a, narrow, grid, (unsigned)g.lds_bytes, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace vf
