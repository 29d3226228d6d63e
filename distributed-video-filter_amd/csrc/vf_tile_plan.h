// vf_tile_plan.h — what the launchers of the neighbourhood kernels (vf_conv.hip, vf_rank.hip) decide
// on the host (host only, no HIP, so tests/tile/tile_plan_check.cc checks it on the CPU).
// Not installed.
#pragma once
#include <stdint.h>

#include <vector>

#include "vf_conv_border.h"

namespace vf {
namespace tile {

constexpr int kTileBytes = 256;  // row bytes of a workgroup's output tile: 16 lanes x 16 B
constexpr int kTileRows = 16;    // rows of a tile: 256 lanes / 16
constexpr int kMaxRows = 65535 * kTileRows;  // output rows of one launch: the grid's y limit

// a kernel or element of kw x kh: odd sides of at most conv::kMaxK
inline bool sides_ok(int kw, int kh) {
  return kw >= 1 && kh >= 1 && kw <= conv::kMaxK && kh <= conv::kMaxK && (kw & 1) && (kh & 1);
}

inline bool border_ok(int border) {
  return border == conv::kReflect101 || border == conv::kReplicate || border == conv::kConstant;
}

// launch_conv's row arguments (vf_internal.h): output rows [y0, y0 + nrows) and source rows
// [s0, s0 + nsrc) of a frame of frame_h rows of width * channels bytes
inline bool rows_ok(const void *src, const void *dst, int width, int channels, int frame_h, int y0, int nrows, int s0,
                    int nsrc) {
  return src && dst && (channels == 1 || channels == 3) && width > 0 && frame_h > 0 && y0 >= 0 && nrows > 0 &&
         y0 + (int64_t)nrows <= frame_h && s0 >= 0 && nsrc > 0 && s0 + (int64_t)nsrc <= frame_h &&
         (uint64_t)width * (uint64_t)channels <= 0x7FFFFFFFull;
}

// the side of the square a kw x kh kernel or element runs in: the kernels are compiled for 3, 5, 7
inline int square_side(int kw, int kh) {
  const int big = kw > kh ? kw : kh;
  return big <= 3 ? 3 : big <= 5 ? 5 : 7;
}

// Where entry (row j, column i) of the kw x kh kernel sits in the ks x ks square, row-major, the
// kernel centred: the positions around it weigh 0 (conv) or are not members (rank).
inline int square_at(int ks, int kw, int kh, int j, int i) {
  return (j + (ks - kh) / 2) * ks + i + (ks - kw) / 2;
}

struct RowChunk {
  int done, m;  // output rows [done, done + m) of the call's nrows
};

// the launches of nrows output rows: in order, each of at most kMaxRows rows
inline std::vector<RowChunk> row_chunks(int nrows) {
  std::vector<RowChunk> out;
  for (int done = 0; done < nrows; done += out.back().m)
    out.push_back(RowChunk{done, nrows - done < kMaxRows ? nrows - done : kMaxRows});
  return out;
}

}  // namespace tile
}  // namespace vf
