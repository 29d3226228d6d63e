// vf_rank.hip — the rank filters on raw frames: cv2.erode, cv2.dilate (a structuring element of
// odd sides up to 7) and cv2.medianBlur (ksize 3 or 5) for uint8 frames of 1 or 3 interleaved
// channels, exact (DESIGN.md 18 has the definition).  No multiply-adds: min / max on packed bytes.
//
// The geometry is vf_conv.hip's.  A workgroup (256 lanes) owns a tile of kTileRows rows x
// kTileBytes row bytes:
//   * staging: the tile with its halo goes into LDS in 16-B pieces, borders resolved in frame
//     coordinates (vf_conv_border.h).  A tap that contributes nothing -- outside the frame under
//     the constant border, which for erode / dilate means "left out of the set" -- is staged as the
//     operation's neutral byte (255 for the minimum, 0 for the maximum), so the inner loop has no
//     border branches;
//   * compute: lane (lx, ly) produces 16 adjacent bytes of row ly.  gfx950 has no per-byte SIMD
//     min / max, so bytes are taken from the window as pairs zero-extended into the 16-bit halves
//     of a dword (v_perm_b32) and compared with v_pk_min_u16 / v_pk_max_u16.
//       erode / dilate  the element is a bit mask of the KS x KS square the kernel is compiled for
//                       (KS = 3, 5, 7), a by-value argument; each bit is tested wave-uniformly;
//       median          a selection network of compare-exchanges (vf_rank_net.h), on 4 output
//                       bytes at a time (two packed registers per value): 25 values for all 16
//                       bytes at once would not fit the register file;
//   * store: as vf_conv.hip's -- 16 B nontemporal when aligned, else dwords or bytes; nothing
//     outside the row or the launch's rows.
// No device allocation; the launch stays asynchronous on the caller's stream.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <cstring>

#include "vf_conv_border.h"
#include "vf_internal.h"
#include "vf_rank_net.h"
#include "vf_stream.h"
#include "vf_tile.h"

namespace vf {

namespace {

using namespace tile;  // the tile geometry, row arguments and window both kernels share (vf_tile.h)

struct RankArgs {
  Rows r;
  uint64_t mask;  // erode / dilate: bit j * KS + i is member (j, i) of the KS x KS square
};

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
typedef unsigned short us4 __attribute__((ext_vector_type(4)));

struct PkOps {  // v_pk_min_u16 / v_pk_max_u16, two per us4
  static __device__ __forceinline__ us4 lo(us4 a, us4 b) { return __builtin_elementwise_min(a, b); }
  static __device__ __forceinline__ us4 hi(us4 a, us4 b) { return __builtin_elementwise_max(a, b); }
};

enum : int { kErode = 0, kDilate = 1, kMedian = 2 };  // VF_RANK_* (include/vfilter.h)

template <int OP, int KS, int C>
__global__ __launch_bounds__(kBlock) void rank_kernel(const RankArgs a) {
  constexpr int R = KS / 2;
  constexpr int SR = kTileRows + 2 * R;
  constexpr uint32_t kNeutral = OP == kErode ? 0xFFu : 0u;  // what a tap outside the set is staged as
  constexpr uint32_t kNeutral4 = kNeutral * 0x01010101u;
  __shared__ __attribute__((aligned(16))) uint8_t lds[SR * kPitch];
  const int tid = (int)threadIdx.x;
  const int64_t tile_x = (int64_t)blockIdx.x * kTileBytes;  // row offset of the tile's first byte
  const int ty0 = a.r.y0 + (int)blockIdx.y * kTileRows;     // frame row of the tile's first row
  const int yend = a.r.y0 + a.r.nrows;

  // ---- stage the tile and its halo, borders resolved ------------------------------------------
  for (int item = tid; item < SR * kPieces; item += kBlock) {
    const int r = item / kPieces, c = item - r * kPieces;
    const int fy_raw = ty0 - R + r;
    u32x4 v;
    v.x = v.y = v.z = v.w = kNeutral4;
    if (fy_raw < yend + R) {  // rows below the last output row's halo are never read
      const int fy = conv::border_index(fy_raw, a.r.h, a.r.border);
      const int sr = fy - a.r.s0;
      if (fy >= 0 && sr >= 0 && sr < a.r.nsrc) {
        const uint8_t *row = a.r.src + (size_t)sr * a.r.row_bytes;
        const int64_t o = tile_x - kHalo + 16 * c;  // row offset of the piece
        if (o >= 0 && o + 16 <= (int64_t)a.r.row_bytes) {
          v = load16_any(row + o);
        } else {
          uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const int64_t off = o + k;
            // floor(off / C) for off >= -kHalo
            const int64_t px = (off + (int64_t)kHalo * C) / C - kHalo;
            uint32_t val = kNeutral;
            if (px >= -R && px < (int64_t)a.r.w + R) {  // only pixels a tap of the frame can reach
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
    uint2 *p = reinterpret_cast<uint2 *>(lds + r * kPitch + 16 * c);  // 8-B aligned (kPitch % 8 == 0)
    p[0] = make_uint2(v.x, v.y);
    p[1] = make_uint2(v.z, v.w);
  }
  __syncthreads();

  // ---- 16 output bytes per lane -----------------------------------------------------------------
  const int lx = tid & 15, ly = tid >> 4;
  const int y = ty0 + ly;
  const int64_t o = tile_x + 16 * lx;
  if (y >= yend || o >= (int64_t)a.r.row_bytes) return;
  uint32_t d[4];
  if constexpr (OP == kMedian) {
    // 4 output bytes at a time: value (j, i) of the group is the 4 window bytes (i - R) * C away
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      us4 v[KS * KS];
#pragma unroll
      for (int j = 0; j < KS; ++j) {
        uint32_t w[16];
        load_window(lds, ly + j, lx, w);  // the dwords no tap of this group uses are dropped
#pragma unroll
        for (int i = 0; i < KS; ++i) {
          const int at = kWinTile + 4 * g + (i - R) * C;
          const us2 p0 = win_pair<us2>(w, at), p1 = win_pair<us2>(w, at + 2);
          v[j * KS + i] = us4{p0.x, p0.y, p1.x, p1.y};
        }
      }
      us4 m;
      if constexpr (KS == 3) m = rank::median9<PkOps>(v);
      else m = rank::median25<PkOps>(v);
      d[g] = pack4(us2{m.x, m.y}, us2{m.z, m.w});
    }
  } else {
    const us2 neutral2 = us2{(unsigned short)kNeutral, (unsigned short)kNeutral};
    us2 acc[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) acc[p] = neutral2;
    const uint64_t mask = a.mask;
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      if (((mask >> (j * KS)) & ((1u << KS) - 1)) == 0) continue;  // a row without members (wave-uniform)
      uint32_t w[16];
      load_window(lds, ly + j, lx, w);
#pragma unroll
      for (int i = 0; i < KS; ++i) {
        if (!((mask >> (j * KS + i)) & 1)) continue;  // wave-uniform: the mask is a kernel argument
#pragma unroll
        for (int p = 0; p < 8; ++p) {
          const us2 t = win_pair<us2>(w, kWinTile + 2 * p + (i - R) * C);
          if constexpr (OP == kErode) acc[p] = __builtin_elementwise_min(acc[p], t);
          else acc[p] = __builtin_elementwise_max(acc[p], t);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) d[m] = pack4(acc[2 * m], acc[2 * m + 1]);
  }

  // ---- store: inside the row and inside the launch's rows only ------------------------------------
  uint8_t *dp = a.r.dst + (size_t)(y - a.r.y0) * a.r.row_bytes + o;
  const int64_t left = (int64_t)a.r.row_bytes - o;
  if (left >= 16 && ((uintptr_t)dp & 15) == 0) {
    u32x4 v;
    v.x = d[0];
    v.y = d[1];
    v.z = d[2];
    v.w = d[3];
    st16<true>(reinterpret_cast<u32x4 *>(dp), v);
  } else if (left >= 16 && ((uintptr_t)dp & 3) == 0) {
    uint32_t *p4 = reinterpret_cast<uint32_t *>(dp);
#pragma unroll
    for (int m = 0; m < 4; ++m) p4[m] = d[m];
  } else {
    const int n = left < 16 ? (int)left : 16;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < n) dp[k] = (uint8_t)(d[k >> 2] >> (8 * (k & 3)));
  }
}

template <int OP, int C>
hipError_t launch_op(int ks, const RankArgs &a, dim3 grid, hipStream_t stream) {
  if (ks == 3) hipLaunchKernelGGL((rank_kernel<OP, 3, C>), grid, dim3(kBlock), 0, stream, a);
  else if (ks == 5) hipLaunchKernelGGL((rank_kernel<OP, 5, C>), grid, dim3(kBlock), 0, stream, a);
  else if constexpr (OP != kMedian) hipLaunchKernelGGL((rank_kernel<OP, 7, C>), grid, dim3(kBlock), 0, stream, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

template <int C>
hipError_t launch_c(int op, int ks, const RankArgs &a, dim3 grid, hipStream_t stream) {
  if (op == kErode) return launch_op<kErode, C>(ks, a, grid, stream);
  if (op == kDilate) return launch_op<kDilate, C>(ks, a, grid, stream);
  return launch_op<kMedian, C>(ks, a, grid, stream);
}

}  // namespace

uint64_t rank_mask(const uint8_t *element, int kw, int kh) {
  uint64_t m = 0;
  for (int i = 0; i < kw * kh; ++i)
    if (element[i]) m |= (uint64_t)1 << i;
  return m;
}

hipError_t launch_rank(const void *dsrc, void *ddst, int width, int channels, int frame_h, int y0, int nrows, int s0,
                       int nsrc, int op, uint64_t mask, int kw, int kh, int border, hipStream_t stream) {
  if (nrows <= 0 || width <= 0) return hipSuccess;
  const uint64_t full = kw >= 1 && kh >= 1 && kw * kh < 64 ? ((uint64_t)1 << (kw * kh)) - 1 : 0;
  if (!rows_ok(dsrc, ddst, width, channels, frame_h, y0, nrows, s0, nsrc) || !sides_ok(kw, kh) || !border_ok(border) ||
      op < kErode || op > kMedian || (mask & full) == 0 || (mask & ~full) != 0)
    return hipErrorInvalidValue;
  if (op == kMedian && (kw != kh || (kw != 3 && kw != 5) || mask != full || border != conv::kReplicate))
    return hipErrorInvalidValue;
  const int ks = square_side(kw, kh);
  RankArgs a;
  std::memset(&a, 0, sizeof a);
  // the added positions of the square are not members
  for (int j = 0; j < kh; ++j)
    for (int i = 0; i < kw; ++i)
      if ((mask >> (j * kw + i)) & 1) a.mask |= (uint64_t)1 << square_at(ks, kw, kh, j, i);
  return launch_rows(&a.r, dsrc, ddst, width, channels, frame_h, y0, nrows, s0, nsrc, border, [&](dim3 grid) {
    return channels == 3 ? launch_c<3>(op, ks, a, grid, stream) : launch_c<1>(op, ks, a, grid, stream);
  });
}

}  // namespace vf
