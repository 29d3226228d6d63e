// vf_conv.hip — the 2-D convolution filter on raw frames: cv2.filter2D(frame, -1, K / 2^shift)
// for uint8 frames of 1 or 3 interleaved channels, integer weights, odd sides up to 7, exact
// (DESIGN.md 16 has the definition).  The first kernel here that reads a pixel's neighbours.
//
// A frame is H rows of W * C bytes and the horizontal neighbour of a byte is C bytes away, so the
// kernel works on bytes and never de-interleaves.  A workgroup (256 lanes) owns a tile of
// kTileRows rows x kTileBytes row bytes:
//   * staging: the tile with its halo, (kTileRows + 2 R) rows x kStageBytes bytes, goes into LDS
//     in 16-B pieces with the borders resolved, in frame coordinates (vf_conv_border.h): a piece
//     that leaves the row is put together byte by byte, so the inner loop has no border branches;
//   * compute: lane (lx, ly) produces 16 adjacent bytes of row ly.  Per kernel row it reads one
//     64-B window of LDS (8-B aligned; the row pitch is 2 banks off a multiple of 64, so the two
//     rows a 32-lane group touches would not collide as b64 reads -- the compiler drops the dwords
//     no tap uses and reads the rest as ds_read2_b32 pairs, which do: DESIGN.md 16.3) and every
//     tap is a compile-time byte of that window;
//   * store: 16 B per lane, nontemporal, when the address is 16-B aligned (always,
//     for W * C a multiple of 16 at an aligned pointer); otherwise dwords or bytes.
// Two arithmetic forms, both exact, chosen on the host from K alone (conv_form):
//   wide    one 32-bit multiply-add per tap and byte;
//   narrow  packed 16-bit multiply-adds on byte pairs, when sum|K| * 255 < 2^15.
// The weights (embedded, centred, in the KS x KS square the kernel is compiled for; KS = 3, 5, 7),
// shift and geometry are by-value kernel arguments: no device allocation, and the launch stays
// asynchronous on the caller's stream.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <cstdlib>
#include <cstring>

#include "vf_conv_border.h"
#include "vf_internal.h"
#include "vf_stream.h"
#include "vf_tile.h"

namespace vf {

namespace {

using namespace tile;  // the tile geometry, row arguments and window both kernels share (vf_tile.h)

struct ConvArgs {
  Rows r;
  int32_t shift;
  int16_t k[conv::kMaxK * conv::kMaxK];  // KS * KS weights, row-major
};

// byte idx (compile time after unrolling) of a window of dwords
__device__ __forceinline__ int win_byte(const uint32_t (&w)[16], int idx) {
  return (int)((w[idx >> 2] >> (8 * (idx & 3))) & 0xFFu);
}

typedef short short2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t finish(int acc, int shift, int bias, int odd) {
  // round half to even: floor((acc + h - 1 + (floor(acc / 2^shift) is odd)) / 2^shift); shift 0: acc
  const int q = (acc + bias + ((acc >> shift) & odd)) >> shift;
  return (uint32_t)min(max(q, 0), 255);
}

template <int KS, int C, bool NARROW>
__global__ __launch_bounds__(kBlock) void conv_kernel(const ConvArgs a) {
  constexpr int R = KS / 2;
  constexpr int SR = kTileRows + 2 * R;
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
    v.x = v.y = v.z = v.w = 0;
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
            uint32_t val = 0;
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
  const int shift = a.shift;
  const int bias = shift ? (1 << (shift - 1)) - 1 : 0, odd = shift ? 1 : 0;
  uint32_t q[16];
  if constexpr (NARROW) {
    short2v acc[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) acc[p] = (short2v)(0);
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      uint32_t w[16];
      load_window(lds, ly + j, lx, w);
#pragma unroll
      for (int i = 0; i < KS; ++i) {
        const short kk = a.k[j * KS + i];
        const short2v k2 = (short2v)(kk);
#pragma unroll
        for (int p = 0; p < 8; ++p) acc[p] += win_pair<short2v>(w, kWinTile + 2 * p + (i - R) * C) * k2;
      }
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      q[2 * p] = finish((int)acc[p].x, shift, bias, odd);
      q[2 * p + 1] = finish((int)acc[p].y, shift, bias, odd);
    }
  } else {
    int acc[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) acc[b] = 0;
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      uint32_t w[16];
      load_window(lds, ly + j, lx, w);
#pragma unroll
      for (int i = 0; i < KS; ++i) {
        const int kk = a.k[j * KS + i];
#pragma unroll
        for (int b = 0; b < 16; ++b) acc[b] += kk * win_byte(w, kWinTile + b + (i - R) * C);
      }
    }
#pragma unroll
    for (int b = 0; b < 16; ++b) q[b] = finish(acc[b], shift, bias, odd);
  }
  uint32_t d[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) d[m] = q[4 * m] | q[4 * m + 1] << 8 | q[4 * m + 2] << 16 | q[4 * m + 3] << 24;

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

template <int KS, int C>
hipError_t launch_ks(const ConvArgs &a, bool narrow, dim3 grid, hipStream_t stream) {
  if (narrow) hipLaunchKernelGGL((conv_kernel<KS, C, true>), grid, dim3(kBlock), 0, stream, a);
  else hipLaunchKernelGGL((conv_kernel<KS, C, false>), grid, dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

template <int C>
hipError_t launch_c(int ks, const ConvArgs &a, bool narrow, dim3 grid, hipStream_t stream) {
  if (ks == 3) return launch_ks<3, C>(a, narrow, grid, stream);
  if (ks == 5) return launch_ks<5, C>(a, narrow, grid, stream);
  return launch_ks<7, C>(a, narrow, grid, stream);
}

}  // namespace

bool conv_narrow_fits(const int16_t *weights, int count) {
  long sum = 0;
  for (int i = 0; i < count; ++i) sum += std::labs((long)weights[i]);
  return sum * 255 < 32768;
}

int conv_form_env() {
  const char *e = std::getenv("VF_CONV_FORM");  // read per call: tests and tools switch it in-process
  if (e && std::strcmp(e, "wide") == 0) return 1;
  if (e && std::strcmp(e, "narrow") == 0) return 2;
  return 0;
}

hipError_t launch_conv(const void *dsrc, void *ddst, int width, int channels, int frame_h, int y0, int nrows, int s0,
                       int nsrc, const int16_t *weights, int kw, int kh, int shift, int border, int form,
                       hipStream_t stream) {
  if (nrows <= 0 || width <= 0) return hipSuccess;
  if (!weights || !rows_ok(dsrc, ddst, width, channels, frame_h, y0, nrows, s0, nsrc) || !sides_ok(kw, kh) ||
      !border_ok(border) || shift < 0 || shift > 16)
    return hipErrorInvalidValue;
  const int ks = square_side(kw, kh);
  ConvArgs a;
  std::memset(&a, 0, sizeof a);
  // the added taps of the square weigh 0, whatever they read
  for (int j = 0; j < kh; ++j)
    for (int i = 0; i < kw; ++i) a.k[square_at(ks, kw, kh, j, i)] = weights[j * kw + i];
  a.shift = shift;
  // the narrow form when it holds the kernel; VF_CONV_FORM=wide forces the other, =narrow changes
  // nothing a kernel the narrow form cannot hold
  const bool narrow = form != 1 && conv_narrow_fits(weights, kw * kh);
  return launch_rows(&a.r, dsrc, ddst, width, channels, frame_h, y0, nrows, s0, nsrc, border, [&](dim3 grid) {
    return channels == 3 ? launch_c<3>(ks, a, narrow, grid, stream) : launch_c<1>(ks, a, narrow, grid, stream);
  });
}

}  // namespace vf
