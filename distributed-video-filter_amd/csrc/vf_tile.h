// vf_tile.h — what the neighbourhood kernels share (vf_conv.hip, vf_rank.hip): a workgroup's
// output tile, its staged image in LDS and a lane's window of it; the row arguments (Rows) and the
// walk over their launches; the 16-B load of any alignment, the window load and the byte pairs taken
// from it.  Each kernel keeps its own staging loop and store: shared, they cost speed or were
// miscompiled.  The host's decisions: vf_tile_plan.h.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vf_internal.h"
#include "vf_stream.h"
#include "vf_tile_plan.h"

namespace vf {
namespace tile {

constexpr int kHalo = 32;                   // LDS position of the tile's first byte (>= 3 * 3, 16-B multiple)
constexpr int kStageBytes = kTileBytes + 2 * kHalo;  // staged bytes per row: 20 pieces of 16 B
constexpr int kPitch = kStageBytes + 8;     // LDS row pitch: 82 dwords = 18 banks mod 64
constexpr int kPieces = kStageBytes / 16;
constexpr int kWin0 = 8;                    // a lane's window starts at lx * 16 + kWin0 ...
constexpr int kWinTile = kHalo - kWin0;     // ... so its first output byte is window byte 24

// The first member of a kernel's by-value argument struct (48 bytes: what follows keeps its offset).
struct Rows {
  const uint8_t *src;  // frame row s0, byte 0
  uint8_t *dst;        // frame row y0, byte 0
  uint32_t row_bytes;  // W * C
  int32_t w, h;        // the frame
  int32_t y0, nrows;   // output rows [y0, y0 + nrows)
  int32_t s0, nsrc;    // source rows present [s0, s0 + nsrc)
  int32_t border;
};
static_assert(sizeof(Rows) == 48, "the arguments after Rows keep their kernarg offsets");

// Host: fill *r for rows that are rows_ok and call launch(grid) once per row chunk, with r->y0,
// r->nrows and r->dst set for it; the first error ends the walk.
template <class F>
inline hipError_t launch_rows(Rows *r, const void *dsrc, void *ddst, int width, int channels, int frame_h, int y0,
                              int nrows, int s0, int nsrc, int border, F launch) {
  r->src = static_cast<const uint8_t *>(dsrc);
  r->row_bytes = (uint32_t)width * (uint32_t)channels;
  r->w = width;
  r->h = frame_h;
  r->s0 = s0;
  r->nsrc = nsrc;
  r->border = border;
  const unsigned gx = (r->row_bytes + kTileBytes - 1) / kTileBytes;
  for (const RowChunk &c : row_chunks(nrows)) {
    r->y0 = y0 + c.done;
    r->nrows = c.m;
    r->dst = static_cast<uint8_t *>(ddst) + (size_t)c.done * r->row_bytes;
    const hipError_t e = launch(dim3(gx, (unsigned)((c.m + kTileRows - 1) / kTileRows)));
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

__device__ __forceinline__ u32x4 load16_any(const uint8_t *p) {
  const uintptr_t a = (uintptr_t)p;
  u32x4 v;
  if ((a & 15) == 0) {
    v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
  } else if ((a & 3) == 0) {
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
    v.x = q[0];
    v.y = q[1];
    v.z = q[2];
    v.w = q[3];
  } else {
    uint32_t d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      d[j] = (uint32_t)p[4 * j] | (uint32_t)p[4 * j + 1] << 8 | (uint32_t)p[4 * j + 2] << 16 | (uint32_t)p[4 * j + 3] << 24;
    v.x = d[0];
    v.y = d[1];
    v.z = d[2];
    v.w = d[3];
  }
  return v;
}

// lane lx's 64-B window of staged row `row` (8-B aligned), as dwords
__device__ __forceinline__ void load_window(const uint8_t *lds, int row, int lx, uint32_t (&w)[16]) {
  const uint2 *rp = reinterpret_cast<const uint2 *>(lds + row * kPitch + 16 * lx + kWin0);
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const uint2 t = rp[m];
    w[2 * m] = t.x;
    w[2 * m + 1] = t.y;
  }
}

// bytes idx and idx + 1 of the window, zero-extended into the two 16-bit halves of T
template <class T>
__device__ __forceinline__ T win_pair(const uint32_t (&w)[16], int idx) {
  const int d = idx >> 2, k = idx & 3;
  uint32_t r;
  if (k < 3) r = __builtin_amdgcn_perm(0u, w[d], 0x0C000C00u | (uint32_t)(k + 1) << 16 | (uint32_t)k);
  else r = __builtin_amdgcn_perm(w[d + 1], w[d], 0x0C040C03u);
  return __builtin_bit_cast(T, r);
}

// the low bytes of two pairs as the four bytes of a dword
template <class T>
__device__ __forceinline__ uint32_t pack4(T a, T b) {
  return __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, b), __builtin_bit_cast(uint32_t, a), 0x06040200u);
}

}  // namespace tile
}  // namespace vf
