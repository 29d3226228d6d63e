// vf_warp.hip — the affine warp on raw frames (cv2.warpAffine with WARP_INVERSE_MAP semantics, and
// cv2.flip): every output pixel reads the source at m * (x, y, 1), in cv2's fixed
// point, nearest or bilinear, under one of three borders.  vf_warp_plan.h holds every rule; this
// file holds the loops.  One launch a frame, the first kernel of the library whose reads are a gather:
//
// warp_kernel   the grid is (tile x, tile y) over the OUTPUT, a tile kTileW pixels by `rows` rows.  A
//     lane owns one output byte column (pixel x, channel c): it computes its two column deltas once,
//     in fp64; the tile's row bases are computed once by the first lanes into LDS and read from there
//     by everyone (wave-uniform); a lane walks its rows, and the stores of a row are consecutive
//     bytes across the waves.  The workgroup takes one of two paths, decided from tile_footprint, the
//     same for all its lanes:
//       interior   the tile's source box lies inside the frame and fits the LDS budget: the box's
//                  rows are staged with 16-byte loads of any alignment (tile::load16_any; the last
//                  piece of the frame's last bytes is read bytewise, nothing past the frame is
//                  touched) and the taps are gathered from LDS without a border rule;
//       general    every other tile (one that touches the border, or a box over the budget as under
//                  a strong shrink): the taps are gathered from global memory through border_at.
//     Both give the same bytes: the taps are the same positions.
// Every access of a pixel outside the staging is one byte a lane; wider accesses on the general
// path, and a permutation kernel for the flips, were not built.  VF_WARP_LDS (the LDS budget in
// bytes; 0 forces the general path everywhere) and VF_WARP_ROWS (a tile's rows) are read at every
// launch, for measurements and for the tests that compare the two paths in one process; DESIGN.md
// 24.4 records what each measured.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "vf_env.h"
#include "vf_internal.h"
#include "vf_tile.h"
#include "vf_warp_plan.h"

namespace vf {

namespace {

constexpr int kTileW = 64;              // output pixels a tile row: a wave's lanes on 1-channel frames
constexpr int kTileRows = 16;           // output rows a tile (VF_WARP_ROWS; kMaxTileRows at the most)
constexpr int kMaxTileRows = 64;
constexpr uint32_t kWarpLds = 16384;    // the staged box's budget in bytes (VF_WARP_LDS)
constexpr uint32_t kMaxWarpLds = 61440;  // with the row bases below 64 KiB: no opt-in to large LDS is needed

struct WarpArg {
  double m[6];        // resolved for the frame
  int32_t W, H;
  int32_t border;
  int32_t rows;       // a tile's rows
  uint32_t value;     // the constant border's bytes: channel c in bits 8 c ..
  uint32_t lds;       // the budget; 0: the general path everywhere
};

// Threads: the tile's byte columns times the row groups that walk its rows side by side.
template <bool C3>
struct Shape {
  static constexpr int C = C3 ? 3 : 1;
  static constexpr int kCols = kTileW * C;      // 64 or 192
  static constexpr int kGroups = C3 ? 2 : 4;
  static constexpr int kThreads = kCols * kGroups;  // 256 or 384
};

template <bool C3, bool LINEAR>
__global__ __launch_bounds__(Shape<C3>::kThreads) void warp_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                                    const WarpArg a) {
  using S = Shape<C3>;
  constexpr int C = S::C;
  constexpr int interp = LINEAR ? warp::kLinear : warp::kNearest;
  extern __shared__ __align__(16) uint8_t staged[];
  __shared__ int32_t bases[2 * kMaxTileRows];  // X0 of the tile's rows, then Y0
  const int t = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * a.rows;
  const int x1 = (x0 + kTileW < a.W ? x0 + kTileW : a.W) - 1, y1 = (y0 + a.rows < a.H ? y0 + a.rows : a.H) - 1;
  if (t <= y1 - y0) {
    const int rd = warp::round_delta(interp);
    bases[t] = warp::row_base(a.m[1], a.m[2], y0 + t, rd);
    bases[kMaxTileRows + t] = warp::row_base(a.m[4], a.m[5], y0 + t, rd);
  }
  // the path: workgroup-uniform, from uniform values only
  const warp::Box b = warp::tile_footprint(a.m, interp, x0, x1, y0, y1);
  const bool inside = b.sx_lo >= 0 && b.sx_hi < a.W && b.sy_lo >= 0 && b.sy_hi < a.H;
  const uint32_t box_bytes = inside ? (uint32_t)(b.sx_hi - b.sx_lo + 1) * C : 0u;
  const uint32_t pitch = (box_bytes + 15u) & ~15u, box_rows = inside ? (uint32_t)(b.sy_hi - b.sy_lo + 1) : 0u;
  const bool lds_path = inside && (uint64_t)pitch * box_rows <= (uint64_t)a.lds;
  if (lds_path) {
    const uint32_t pieces = pitch >> 4, total = pieces * box_rows;
    const uint64_t frame_bytes = (uint64_t)a.W * (uint64_t)a.H * C;
    for (uint32_t i = (uint32_t)t; i < total; i += S::kThreads) {
      const uint32_t r = i / pieces, p = i - r * pieces;
      const uint64_t off = ((uint64_t)(b.sy_lo + (int)r) * (uint64_t)a.W + (uint64_t)b.sx_lo) * C + 16u * p;
      u32x4 v;
      if (off + 16 <= frame_bytes) {
        v = tile::load16_any(src + off);
      } else {  // the frame's last bytes: nothing past them is read
        uint32_t d[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < 16 && off + j < frame_bytes; ++j) d[j >> 2] |= (uint32_t)src[off + j] << (8 * (j & 3));
        v.x = d[0], v.y = d[1], v.z = d[2], v.w = d[3];
      }
      *reinterpret_cast<u32x4 *>(staged + (size_t)r * pitch + 16u * p) = v;
    }
  }
  __syncthreads();
  const int col = t % S::kCols, group = t / S::kCols;
  const int x = x0 + col / C, c = col - (col / C) * C;
  if (x > x1) return;
  const int adelta = warp::col_delta(a.m[0], x), bdelta = warp::col_delta(a.m[3], x);  // once a lane, not a row
  const uint32_t value = (a.value >> (8 * c)) & 255u;
  const size_t row_bytes = (size_t)a.W * C;
  uint8_t *out = dst + (size_t)x * C + c;
  if (lds_path) {
    for (int r = group; y0 + r <= y1; r += S::kGroups) {
      const warp::Coord cx = warp::warp_coord(bases[r], adelta, interp);
      const warp::Coord cy = warp::warp_coord(bases[kMaxTileRows + r], bdelta, interp);
      // tile_footprint: both differences are inside the box
      const uint8_t *p = staged + ((uint32_t)(cy.s - b.sy_lo) * pitch + (uint32_t)(cx.s - b.sx_lo) * C + (uint32_t)c);
      uint32_t v;
      if (LINEAR)
        v = warp::warp_blend(p[0], p[C], p[pitch], p[pitch + C], warp::warp_weights(cx.f, cy.f));
      else
        v = p[0];
      out[(size_t)(y0 + r) * row_bytes] = (uint8_t)v;
    }
  } else {
    for (int r = group; y0 + r <= y1; r += S::kGroups) {
      const warp::Coord cx = warp::warp_coord(bases[r], adelta, interp);
      const warp::Coord cy = warp::warp_coord(bases[kMaxTileRows + r], bdelta, interp);
      out[(size_t)(y0 + r) * row_bytes] = (uint8_t)warp::warp_pixel(src, a.W, a.H, C, c, cx, cy, interp, a.border, value);
    }
  }
}

template <bool C3, bool LINEAR>
hipError_t launch_as(const uint8_t *src, uint8_t *dst, const WarpArg &a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.W + kTileW - 1) / kTileW), (unsigned)((a.H + a.rows - 1) / a.rows));
  hipLaunchKernelGGL((warp_kernel<C3, LINEAR>), grid, dim3(Shape<C3>::kThreads), a.lds, stream, src, dst, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_warp(const void *dsrc, void *ddst, int width, int height, int channels, const double *m, int mode,
                       int interp, int border, const uint8_t *value, hipStream_t stream) {
  if (width == 0 || height == 0) return hipSuccess;
  std::string why;
  const int v3[3] = {value ? value[0] : -1, value ? value[1] : -1, value ? value[2] : -1};
  if (!dsrc || !ddst || width < 0 || height < 0 || !warp::limits_ok(m, mode, interp, border, v3, channels, &why) ||
      !warp::frame_ok((uint64_t)width, (uint64_t)height, mode, m, &why))
    return hipErrorInvalidValue;
  WarpArg a;
  warp::resolve(mode, m, width, height, a.m);
  a.W = width, a.H = height, a.border = border;
  a.value = (uint32_t)value[0] | (uint32_t)value[1] << 8 | (uint32_t)value[2] << 16;
  const size_t lds = env_size("VF_WARP_LDS", kWarpLds), rows = env_size("VF_WARP_ROWS", kTileRows);
  a.lds = (uint32_t)(lds > kMaxWarpLds ? kMaxWarpLds : lds) & ~15u;
  a.rows = (int32_t)(rows < 1 ? 1 : rows > (size_t)kMaxTileRows ? (size_t)kMaxTileRows : rows);
  if ((height + a.rows - 1) / a.rows > 65535) a.rows = kMaxTileRows;  // never: a side is at most 32767
  const uint8_t *src = static_cast<const uint8_t *>(dsrc);
  uint8_t *dst = static_cast<uint8_t *>(ddst);
  if (channels == 3)
    return interp == warp::kLinear ? launch_as<true, true>(src, dst, a, stream) : launch_as<true, false>(src, dst, a, stream);
  return interp == warp::kLinear ? launch_as<false, true>(src, dst, a, stream) : launch_as<false, false>(src, dst, a, stream);
}

}  // namespace vf
