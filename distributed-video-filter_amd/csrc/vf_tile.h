// vf_tile.h — the tile geometry the neighbourhood kernels share (vf_conv.hip, vf_rank.hip): a
// workgroup's output tile, its staged image in LDS and a lane's window of it, and the 16-B load of
// any alignment the staging uses.  Each kernel keeps its own staging loop.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vf_internal.h"
#include "vf_stream.h"

namespace vf {
namespace tile {

constexpr int kTileBytes = kConvTileBytes;  // row bytes of a tile: 16 lanes x 16 B
constexpr int kTileRows = kConvTileRows;    // rows of a tile: 256 lanes / 16
constexpr int kHalo = 32;                   // LDS position of the tile's first byte (>= 3 * 3, 16-B multiple)
constexpr int kStageBytes = kTileBytes + 2 * kHalo;  // staged bytes per row: 20 pieces of 16 B
constexpr int kPitch = kStageBytes + 8;     // LDS row pitch: 82 dwords = 18 banks mod 64
constexpr int kPieces = kStageBytes / 16;
constexpr int kWin0 = 8;                    // a lane's window starts at lx * 16 + kWin0 ...
constexpr int kWinTile = kHalo - kWin0;     // ... so its first output byte is window byte 24

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

}  // namespace tile
}  // namespace vf
