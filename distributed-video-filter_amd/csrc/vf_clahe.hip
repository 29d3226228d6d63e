// vf_clahe.hip — CLAHE on raw frames (cv2.createCLAHE(clip, grid).apply on 8-bit input; DESIGN.md
// 23): the frame, extended to whole tiles by reflection, is cut into tiles_x x tiles_y tiles; every
// tile and channel gets a 256-entry table from the tile's clipped and redistributed histogram; a
// pixel is the blend of the four nearest tiles' tables at its value.  vf_clahe_plan.h holds every
// rule; this file holds the loops.  Per frame a memset of the tiles' histogram words and three
// launches:
//
// clahe_hist_kernel    the grid is (row slice, tile): a workgroup counts some rows of one tile into
//     an LDS histogram of channels x 256 bins in R replicas (vf_level.hip's layout: the replicas of
//     a bin are neighbouring words and a lane adds to replica lane % R, so a flat tile spreads over R
//     banks), then adds its non-zero bins to the tile's words in global memory with relaxed
//     agent-scope atomics.  Columns and rows past the frame read their reflection.  The slices are
//     as many as fill the chip from one frame (kHistTarget workgroups), never more than a tile's
//     rows.  A channel outside the mask is not counted.
// clahe_table_kernel   one wave per tile and masked channel: a lane holds four bins (one 16-byte
//     load), clips them, the wave sums the kept counts (the excess is the area less that sum: a
//     tile's bins sum to its area), every bin takes clahe_bin, a wave scan (level_stage's six
//     shuffles) gives the running sums and a lane writes its four clahe_entry as one dword.
// clahe_apply_kernel   the grid is (row strip, cell x, cell y), a cell the pixels between
//     neighbouring tile centres, whose four tiles are the same: cell_start finds the cell's first
//     column and row with the float arithmetic the pixels use, so the rule, not an integer
//     shortcut, decides which pixel belongs to which cell.  The workgroup stages the four tiles'
//     tables (4 x channels x 256 bytes) in LDS; a lane computes its column's weights once and walks
//     the strip's rows: four LDS byte reads and clahe_pixel per byte.  A channel outside the mask is
//     copied.
// Every load and store of a pixel is one byte a lane, consecutive across a wave; the histogram
// keeps four rows of a lane's column in flight at once; wider accesses were not built.  VF_CLAHE_REPLICAS (1, 4, 8),
// VF_CLAHE_HIST_WGS and VF_CLAHE_APPLY_WGS (the workgroups a frame is cut into) are read once, for
// measurements; DESIGN.md 23.4 records what each measured.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "vf_clahe_plan.h"
#include "vf_env.h"
#include "vf_internal.h"

namespace vf {

namespace {

constexpr int kClaheReplicas = 8;    // LDS histograms per workgroup (24 KiB on 3 channels)
constexpr int kHistTarget = 1024;    // clahe_hist_kernel's workgroups a frame: 4 a CU
constexpr int kApplyTarget = 512;    // clahe_apply_kernel's: 1024 .. 8192 measured slower
constexpr uint32_t kRows = 4;        // clahe_hist_kernel: the rows of a lane's column whose loads are in flight at once

struct ClaheArg {
  uint32_t W, H;         // the frame
  uint32_t tw, th;       // a tile of the extended frame
  int tiles_x, tiles_y;
  int mask;              // resolved, no bit beyond the channels
  uint32_t rows;         // hist: the rows of a slice; apply: the strips a cell is cut into
  uint32_t clip;         // table: the clip in counts, capped at the area; 0: none
  uint32_t area;
};

__device__ __forceinline__ void lds_inc(uint32_t *p) {  // result unused: a non-returning ds_add_u32
  (void)__hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// hist: tiles x C x 256 words, added to.
template <bool C3, int R>
__global__ __launch_bounds__(kBlock) void clahe_hist_kernel(const uint8_t *__restrict__ src, uint32_t *__restrict__ hist,
                                                            const ClaheArg a) {
  constexpr uint32_t C = C3 ? 3 : 1;
  constexpr int BINS = C3 ? 768 : 256;
  __shared__ uint32_t s[BINS * R];
  const uint32_t t = threadIdx.x;
  const uint32_t tile = blockIdx.y, tx = tile % (uint32_t)a.tiles_x, ty = tile / (uint32_t)a.tiles_x;
  const uint32_t r0 = blockIdx.x * a.rows;  // of the tile; workgroup-uniform
  if (r0 >= a.th) return;
  const uint32_t r1 = r0 + a.rows < a.th ? r0 + a.rows : a.th;
  for (int i = (int)t; i < BINS * R; i += kBlock) s[i] = 0;
  __syncthreads();
  const uint32_t rep = t & (R - 1);
  const uint32_t x0 = tx * a.tw, y0 = ty * a.th;
  const uint32_t row_bytes = a.tw * C;
  for (uint32_t b = t; b < row_bytes; b += kBlock) {  // a lane's bytes of every row: one column, one channel
    const uint32_t px = b / C, c = b - px * C;
    if (!((a.mask >> c) & 1)) continue;
    const uint32_t x = clahe::source_index(x0 + px, a.W);
    const uint8_t *col = src + ((uint64_t)x * C + c);
    for (uint32_t r = r0; r < r1; r += kRows) {  // kRows loads in flight; a row past the slice re-reads its last row
      uint32_t v[kRows];
#pragma unroll
      for (uint32_t j = 0; j < kRows; ++j) {
        const uint32_t y = clahe::source_index(y0 + (r + j < r1 ? r + j : r1 - 1), a.H);
        v[j] = col[(uint64_t)y * a.W * C];
      }
#pragma unroll
      for (uint32_t j = 0; j < kRows; ++j)
        if (r + j < r1) lds_inc(s + ((c << 8 | v[j]) * R + rep));  // workgroup-uniform
    }
  }
  __syncthreads();
  uint32_t *out = hist + (size_t)tile * BINS;
  for (int b = (int)t; b < BINS; b += kBlock) {
    uint32_t sum = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) sum += s[b * R + r];
    if (sum) (void)__hip_atomic_fetch_add(out + b, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// hist: tiles x C x 256 words (16-byte aligned); tables: tiles x C x 256 bytes (4-byte aligned).
// One wave per (tile, channel); n = tiles x C of them.
template <bool C3>
__global__ __launch_bounds__(kBlock) void clahe_table_kernel(const uint32_t *__restrict__ hist, uint8_t *__restrict__ tables,
                                                             uint32_t n, const ClaheArg a) {
  constexpr uint32_t C = C3 ? 3 : 1;
  const uint32_t lane = threadIdx.x & 63, id = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);  // id: wave-uniform
  if (id >= n) return;
  const uint32_t c = id % C;
  if (!((a.mask >> c) & 1)) return;  // no table: the apply pass copies the channel
  const uint4 q = reinterpret_cast<const uint4 *>(hist)[(size_t)id * 64 + lane];
  uint32_t h[4] = {q.x, q.y, q.z, q.w};
  clahe::Spread sp = {0, 0, 1};
  if (a.clip) {
    uint32_t kept = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) kept += h[j] > a.clip ? a.clip : h[j];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) kept += __shfl_xor(kept, d);
    sp = clahe::spread_of(a.area - kept);  // the bins sum to the area
  }
  uint32_t cum[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t g = clahe::clahe_bin(h[j], a.clip, sp.batch, sp.residual, sp.step, 4 * lane + j);
    cum[j] = j ? cum[j - 1] + g : g;
  }
  uint32_t incl = cum[3];  // the wave's inclusive scan of the lanes' sums
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d);
    if ((int)lane >= d) incl += up;
  }
  const uint32_t excl = incl - cum[3];
  const float scale = clahe::clahe_scale(a.area);
  uint32_t packed = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) packed |= clahe::clahe_entry(cum[j] + excl, scale) << (8 * j);
  reinterpret_cast<uint32_t *>(tables)[(size_t)id * 64 + lane] = packed;
}

// The grid is (strip, cell x, cell y): cell k of an axis holds the pixels whose floor(txf) is k - 1.
template <bool C3>
__global__ __launch_bounds__(kBlock) void clahe_apply_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                             const uint8_t *__restrict__ tables, const ClaheArg a) {
  constexpr uint32_t C = C3 ? 3 : 1;
  __shared__ uint32_t s[4 * C * 64];  // slot q = 2 * (second row tile) + (second column tile), then the channel
  const uint32_t t = threadIdx.x;
  const int kx = (int)blockIdx.y - 1, ky = (int)blockIdx.z - 1;  // floor(txf) of the cell's pixels
  const float inv_x = clahe::clahe_inv(a.tw), inv_y = clahe::clahe_inv(a.th);
  const uint32_t xlo = clahe::cell_start(kx, a.tw, inv_x, a.tiles_x, a.W);
  const uint32_t xhi = clahe::cell_start(kx + 1, a.tw, inv_x, a.tiles_x, a.W);
  const uint32_t ylo = clahe::cell_start(ky, a.th, inv_y, a.tiles_y, a.H);
  const uint32_t yhi = clahe::cell_start(ky + 1, a.th, inv_y, a.tiles_y, a.H);
  if (xlo >= xhi || ylo >= yhi) return;  // an empty cell: workgroup-uniform
  const uint32_t per = (yhi - ylo + a.rows - 1) / a.rows;  // rows a strip
  const uint32_t y0 = ylo + blockIdx.x * per;
  if (y0 >= yhi) return;
  const uint32_t y1 = y0 + per < yhi ? y0 + per : yhi;
  const int tx1 = kx > 0 ? kx : 0, tx2 = kx + 1 < a.tiles_x - 1 ? kx + 1 : a.tiles_x - 1;
  const int ty1 = ky > 0 ? ky : 0, ty2 = ky + 1 < a.tiles_y - 1 ? ky + 1 : a.tiles_y - 1;
  for (uint32_t i = t; i < 4 * C * 64; i += kBlock) {
    const uint32_t q = i / (C * 64), rest = i - q * (C * 64), c = rest >> 6;
    const uint32_t tile = (uint32_t)((q & 2 ? ty2 : ty1) * a.tiles_x + (q & 1 ? tx2 : tx1));
    s[i] = (a.mask >> c) & 1 ? reinterpret_cast<const uint32_t *>(tables)[((size_t)tile * C + c) * 64 + (rest & 63)] : 0u;
  }
  __syncthreads();
  const uint8_t *lut = reinterpret_cast<const uint8_t *>(s);
  const uint32_t row_bytes = (xhi - xlo) * C;
  const uint64_t pitch = (uint64_t)a.W * C;
  for (uint32_t b = t; b < row_bytes; b += kBlock) {
    const uint32_t px = b / C, c = b - px * C;
    const uint64_t at = (uint64_t)(xlo + px) * C + c;
    if (!((a.mask >> c) & 1)) {
      for (uint32_t y = y0; y < y1; ++y) dst[y * pitch + at] = src[y * pitch + at];
      continue;
    }
    const clahe::Weights wx = clahe::clahe_weights(xlo + px, inv_x, a.tiles_x);  // once a lane, not a row
    const uint8_t *l = lut + c * 256;
    for (uint32_t y = y0; y < y1; ++y) {  // one row at a time: four rows' loads in flight measured slower here
      const clahe::Weights wy = clahe::clahe_weights(y, inv_y, a.tiles_y);
      const uint32_t v = src[y * pitch + at];
      dst[y * pitch + at] = (uint8_t)clahe::clahe_pixel(l[v], l[C * 256 + v], l[2 * C * 256 + v], l[3 * C * 256 + v], wx.a,
                                                        wx.a1, wy.a, wy.a1);
    }
  }
}

template <bool C3, int R>
hipError_t launch_hist_as(const uint8_t *src, uint32_t *hist, const ClaheArg &a, uint32_t slices, hipStream_t stream) {
  hipLaunchKernelGGL((clahe_hist_kernel<C3, R>), dim3(slices, (unsigned)(a.tiles_x * a.tiles_y)), dim3(kBlock), 0, stream, src,
                     hist, a);
  return hipGetLastError();
}

template <bool C3>
hipError_t launch_all(const uint8_t *src, uint8_t *dst, uint32_t *hist, uint8_t *tables, ClaheArg a, hipStream_t stream) {
  static const size_t reps = env_size("VF_CLAHE_REPLICAS", kClaheReplicas);
  static const size_t hist_wgs = env_size("VF_CLAHE_HIST_WGS", kHistTarget);
  static const size_t apply_wgs = env_size("VF_CLAHE_APPLY_WGS", kApplyTarget);
  const uint32_t tiles = (uint32_t)(a.tiles_x * a.tiles_y);
  // the histogram: as many slices a tile as make hist_wgs workgroups, at most a tile's rows
  uint32_t slices = (uint32_t)((hist_wgs + tiles - 1) / tiles);
  if (slices < 1) slices = 1;
  if (slices > a.th) slices = a.th;
  if (slices > 65535) slices = 65535;
  a.rows = (a.th + slices - 1) / slices;
  slices = (a.th + a.rows - 1) / a.rows;
  hipError_t e = reps == 1   ? launch_hist_as<C3, 1>(src, hist, a, slices, stream)
                 : reps == 4 ? launch_hist_as<C3, 4>(src, hist, a, slices, stream)
                             : launch_hist_as<C3, kClaheReplicas>(src, hist, a, slices, stream);
  if (e != hipSuccess) return e;
  const uint32_t n = tiles * (C3 ? 3u : 1u);
  hipLaunchKernelGGL(clahe_table_kernel<C3>, dim3((n + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, stream, hist,
                     tables, n, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // the blend: as many strips a cell as make apply_wgs workgroups, at most a tile's rows
  const uint32_t cells = (uint32_t)((a.tiles_x + 1) * (a.tiles_y + 1));
  uint32_t strips = (uint32_t)((apply_wgs + cells - 1) / cells);
  if (strips < 1) strips = 1;
  if (strips > a.th) strips = a.th;
  if (strips > 65535) strips = 65535;
  a.rows = strips;
  hipLaunchKernelGGL(clahe_apply_kernel<C3>, dim3(strips, (unsigned)(a.tiles_x + 1), (unsigned)(a.tiles_y + 1)), dim3(kBlock), 0,
                     stream, src, dst, tables, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_clahe(const void *dsrc, void *ddst, int width, int height, int channels, int clip_q8, int tiles_x,
                        int tiles_y, int mask, void *scratch, hipStream_t stream) {
  if (width == 0 || height == 0) return hipSuccess;
  std::string why;
  if (!dsrc || !ddst || !scratch || ((uintptr_t)scratch & 15) || width < 0 || height < 0 ||
      !clahe::limits_ok(clip_q8, tiles_x, tiles_y, mask, channels, &why) ||
      !clahe::frame_ok((uint64_t)width, (uint64_t)height, tiles_x, tiles_y, &why))
    return hipErrorInvalidValue;
  const clahe::Geometry g = clahe::geometry((uint32_t)width, (uint32_t)height, tiles_x, tiles_y);
  ClaheArg a;
  a.W = (uint32_t)width, a.H = (uint32_t)height, a.tw = g.tw, a.th = g.th;
  a.tiles_x = tiles_x, a.tiles_y = tiles_y;
  a.mask = clahe::resolved_mask(mask, channels);
  a.rows = 1;
  a.area = (uint32_t)g.area;
  const uint64_t clip = clip_q8 > 0 ? clahe::clip_of(clip_q8, g.area) : 0;
  a.clip = (uint32_t)(clip > g.area ? g.area : clip);  // no bin exceeds the area
  const size_t words = clahe::hist_words(tiles_x, tiles_y, channels);
  uint32_t *hist = static_cast<uint32_t *>(scratch);
  uint8_t *tables = reinterpret_cast<uint8_t *>(hist + words);
  const hipError_t e = hipMemsetAsync(hist, 0, words * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  const uint8_t *src = static_cast<const uint8_t *>(dsrc);
  uint8_t *dst = static_cast<uint8_t *>(ddst);
  return channels == 3 ? launch_all<true>(src, dst, hist, tables, a, stream)
                       : launch_all<false>(src, dst, hist, tables, a, stream);
}

}  // namespace vf
