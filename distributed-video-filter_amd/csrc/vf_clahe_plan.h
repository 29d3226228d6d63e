// vf_clahe_plan.h — what CLAHE (vf_clahe.hip; cv2.createCLAHE(...).apply on 8-bit frames; DESIGN.md
// 23) decides outside its loops: the limits of its arguments, the geometry of the tile grid, the
// layout of a VF_STEP_CLAHE step's data, the scratch a step needs, and THE RULES: from a tile's
// 256-bin histogram to its 256-entry table (clip, redistribute, scale), from a pixel's coordinate
// to its two tiles and weights on an axis, and from four table entries to the pixel.  The rules'
// text compiles for the host (no HIP include is needed: tests/clahe/clahe_plan_check.cc checks it on
// the CPU, built with -ffp-contract=off) and for the device, where the kernels call the same
// clahe_bin, clahe_entry, clahe_weights and clahe_pixel.  Every float operation is one separately
// rounded IEEE single-precision operation: nothing is fused (rounded_mul and its kin).  Not installed.
#pragma once
#include <stdint.h>

#include "vf_conv_border.h"

#if defined(__HIPCC__)
#define VF_CLAHE_FN __host__ __device__ inline
#else
#define VF_CLAHE_FN inline
#endif
// A product, a sum or a difference whose result feeds another must not be contracted into a fused
// multiply-add.  HIP's __fmul_rn, __fadd_rn and __fsub_rn are plain operators unless the device
// library's rounded operations are switched on, and the compiler's default lets it fuse across
// them, so each operation here is a function of its own with contraction switched off (the HIP
// compiler honours the pragma under its default -ffp-contract=fast-honor-pragmas; the CPU check is
// built with -ffp-contract=off).
#if defined(__clang__)
#define VF_CLAHE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define VF_CLAHE_NO_CONTRACT
#endif
#define VF_CLAHE_FMUL(a, b) ::vf::clahe::rounded_mul((a), (b))
#define VF_CLAHE_FADD(a, b) ::vf::clahe::rounded_add((a), (b))
#define VF_CLAHE_FSUB(a, b) ::vf::clahe::rounded_sub((a), (b))
#if defined(__HIP_DEVICE_COMPILE__)
// correctly rounded whatever the compiler flags say about fast math
#define VF_CLAHE_U2F(x) __uint2float_rn(x)
#define VF_CLAHE_FDIV(a, b) __fdiv_rn((a), (b))
#define VF_CLAHE_F2I(x) __float2int_rn(x)
#define VF_CLAHE_FLOOR(x) __float2int_rd(x)
#else
#include <cmath>
// IEEE single precision on the host: the conversion rounds to nearest even, the divide is a single
// operation, nearbyint rounds half to even in the default rounding mode.
#define VF_CLAHE_U2F(x) ((float)(uint32_t)(x))
#define VF_CLAHE_FDIV(a, b) ((float)(a) / (float)(b))
#define VF_CLAHE_F2I(x) ((int)std::nearbyint(x))
#define VF_CLAHE_FLOOR(x) ((int)std::floor(x))
#endif

#include <string>

namespace vf {
namespace clahe {

VF_CLAHE_FN float rounded_mul(float a, float b) {
  VF_CLAHE_NO_CONTRACT
  const float r = a * b;
  return r;
}
VF_CLAHE_FN float rounded_add(float a, float b) {
  VF_CLAHE_NO_CONTRACT
  const float r = a + b;
  return r;
}
VF_CLAHE_FN float rounded_sub(float a, float b) {
  VF_CLAHE_NO_CONTRACT
  const float r = a - b;
  return r;
}

constexpr int kMaxTilesAxis = 16;               // tiles_x, tiles_y: 1 .. 16
constexpr int kMaxTiles = kMaxTilesAxis * kMaxTilesAxis;
constexpr int kMaxClipQ8 = 1 << 24;             // clip_q8: the clip limit in units of 1 / 256; 0: no clipping
constexpr uint64_t kMaxPixels = 0xFFFFFFFFull;  // of a frame
constexpr uint64_t kMaxSide = 1ull << 30;       // of a frame: a padded coordinate fits an int
constexpr uint64_t kMaxArea = 0x7FFFFFFFull;    // of a tile of the extended frame: every count fits 31 bits
constexpr int kStepData = 4;                    // a VF_STEP_CLAHE step's data: {mask, clip_q8, tiles_x, tiles_y} as int32
// The scratch of one step: the tiles' histogram words, tiles x channels x 256 uint32, then their
// tables, as many bytes.  At most 960 KiB.
constexpr size_t kHistWords = (size_t)kMaxTiles * 3 * 256;
constexpr size_t kTableBytes = (size_t)kMaxTiles * 3 * 256;
constexpr size_t kScratchBytes = kHistWords * sizeof(uint32_t) + kTableBytes;

inline size_t hist_words(int tiles_x, int tiles_y, int channels) { return (size_t)tiles_x * tiles_y * channels * 256; }
inline size_t table_bytes(int tiles_x, int tiles_y, int channels) { return (size_t)tiles_x * tiles_y * channels * 256; }

// ---- geometry ----------------------------------------------------------------------------------------

// The extended frame and its tiles.  When both axes divide, the frame itself; else it is padded
// (reflect-101) on the right by tiles_x - W % tiles_x and at the bottom by tiles_y - H % tiles_y:
// a full tiles_x when only the height fails to divide, and the other way round, as cv2 does.
struct Geometry {
  uint32_t We, He;  // the extended frame
  uint32_t tw, th;  // a tile
  uint64_t area;    // tw * th
};

VF_CLAHE_FN Geometry geometry(uint32_t W, uint32_t H, int tiles_x, int tiles_y) {
  Geometry g;
  const uint32_t tx = (uint32_t)tiles_x, ty = (uint32_t)tiles_y;
  if (W % tx == 0 && H % ty == 0) {
    g.We = W, g.He = H;
  } else {
    g.We = W + (tx - W % tx), g.He = H + (ty - H % ty);
  }
  g.tw = g.We / tx, g.th = g.He / ty;
  g.area = (uint64_t)g.tw * g.th;
  return g;
}

// The frame's coordinate that position p of the extended frame's axis reads (n >= 1 frame elements).
VF_CLAHE_FN uint32_t source_index(uint32_t p, uint32_t n) {
  return p < n ? p : (uint32_t)conv::border_index((int)p, (int)n, conv::kReflect101);
}

// ---- the table rule ----------------------------------------------------------------------------------

// The clip of a tile in counts: max((clip_q8 * area) >> 16, 1) in 64 bits; clip_q8 > 0.
VF_CLAHE_FN uint64_t clip_of(int clip_q8, uint64_t area) {
  const uint64_t c = ((uint64_t)clip_q8 * area) >> 16;
  return c < 1 ? 1 : c;
}

// What the redistribution adds, from the excess above the clip.
struct Spread {
  uint32_t batch, residual, step;
};

VF_CLAHE_FN Spread spread_of(uint32_t excess) {
  Spread s;
  s.batch = excess / 256;
  s.residual = excess - 256 * s.batch;
  s.step = s.residual ? (256 / s.residual > 1 ? 256 / s.residual : 1) : 1;
  return s;
}

// Bin v after clipping and redistribution.  clip: clip_of's, or 0 for no clipping (batch and
// residual are 0 then).  Bin v gains 1 exactly when v % step == 0 and v / step < residual.
VF_CLAHE_FN uint32_t clahe_bin(uint32_t h_v, uint64_t clip, uint32_t batch, uint32_t residual, uint32_t step, uint32_t v) {
  if (clip == 0) return h_v;
  const uint32_t kept = (uint64_t)h_v > clip ? (uint32_t)clip : h_v;
  const uint32_t extra = (residual > 0 && v % step == 0 && v / step < residual) ? 1u : 0u;
  return kept + batch + extra;
}

// 255.0f / (float)area: one divide.
VF_CLAHE_FN float clahe_scale(uint64_t area) { return VF_CLAHE_FDIV(255.0f, VF_CLAHE_U2F((uint32_t)area)); }

// table[v] from cum = the redistributed bins 0 .. v summed: one conversion, one multiply, half to even.
VF_CLAHE_FN uint32_t clahe_entry(uint32_t cum, float scale) {
  const int r = VF_CLAHE_F2I(VF_CLAHE_FMUL(VF_CLAHE_U2F(cum), scale));
  return (uint32_t)(r < 0 ? 0 : r > 255 ? 255 : r);
}

// The rule as one function: a tile's histogram h (its sum is area, 1 .. 2^31 - 1) to its table.
VF_CLAHE_FN void clahe_table(const uint32_t h[256], uint64_t area, uint64_t clip, uint8_t out[256]) {
  uint64_t excess = 0;
  if (clip)
    for (int v = 0; v < 256; ++v)
      if ((uint64_t)h[v] > clip) excess += (uint64_t)h[v] - clip;
  const Spread s = spread_of((uint32_t)excess);
  const float scale = clahe_scale(area);
  uint32_t cum = 0;
  for (uint32_t v = 0; v < 256; ++v) {
    cum += clahe_bin(h[v], clip, s.batch, s.residual, s.step, v);
    out[v] = (uint8_t)clahe_entry(cum, scale);
  }
}

// ---- the interpolation -------------------------------------------------------------------------------

// A pixel's two tiles and weights on one axis.
struct Weights {
  int t1, t2;    // clamped to 0 .. tiles - 1
  int raw;       // floor(txf): t1 before the clamp, -1 .. tiles - 1
  float a, a1;   // the weight of t2 and of t1
};

// inv = 1.0f / (float)tile_side (clahe_inv).
VF_CLAHE_FN float clahe_inv(uint32_t side) { return VF_CLAHE_FDIV(1.0f, VF_CLAHE_U2F(side)); }

VF_CLAHE_FN Weights clahe_weights(uint32_t x, float inv, int tiles) {
  Weights w;
  const float txf = VF_CLAHE_FSUB(VF_CLAHE_FMUL(VF_CLAHE_U2F(x), inv), 0.5f);
  const int t = VF_CLAHE_FLOOR(txf);
  w.raw = t;
  w.a = VF_CLAHE_FSUB(txf, (float)t);
  w.a1 = VF_CLAHE_FSUB(1.0f, w.a);
  w.t2 = t + 1 < tiles - 1 ? t + 1 : tiles - 1;
  w.t1 = t > 0 ? t : 0;
  return w;
}

// (T11 xa1 + T12 xa) ya1 + (T21 xa1 + T22 xa) ya, every product and every sum rounded, then half to
// even and the clamp.  T11 = T[ty1][tx1][s], T12 = T[ty1][tx2][s], T21 = T[ty2][tx1][s], T22 = T[ty2][tx2][s].
VF_CLAHE_FN uint32_t clahe_pixel(uint32_t t11, uint32_t t12, uint32_t t21, uint32_t t22, float xa, float xa1, float ya,
                                 float ya1) {
  const float top = VF_CLAHE_FADD(VF_CLAHE_FMUL((float)t11, xa1), VF_CLAHE_FMUL((float)t12, xa));
  const float bot = VF_CLAHE_FADD(VF_CLAHE_FMUL((float)t21, xa1), VF_CLAHE_FMUL((float)t22, xa));
  const float res = VF_CLAHE_FADD(VF_CLAHE_FMUL(top, ya1), VF_CLAHE_FMUL(bot, ya));
  const int r = VF_CLAHE_F2I(res);
  return (uint32_t)(r < 0 ? 0 : r > 255 ? 255 : r);
}

// The first x of an axis of n frame elements whose floor(txf) is at least k, n when none is: the
// interpolation cells' boundaries.  floor(txf) never falls as x rises (a conversion, a product with
// a positive number, a difference and a floor are each monotone), so the search starts at the
// position the exact arithmetic gives, ((2 k + 1) side + 1) / 2, and walks the step or two that
// rounding can move it.
VF_CLAHE_FN uint32_t cell_start(int k, uint32_t side, float inv, int tiles, uint32_t n) {
  if (k < 0) return 0;
  const uint64_t nominal = ((uint64_t)(2 * k + 1) * side + 1) / 2;
  uint32_t b = nominal > n ? n : (uint32_t)nominal;
  while (b > 0 && clahe_weights(b - 1, inv, tiles).raw >= k) --b;
  while (b < n && clahe_weights(b, inv, tiles).raw < k) ++b;
  return b;
}

// ---- limits (host) -----------------------------------------------------------------------------------

// The mask with 0 resolved to all of the frame's channels.
inline int resolved_mask(int mask, int channels) { return mask == 0 ? (1 << channels) - 1 : mask; }

// The filter arguments of every entry point and of a VF_STEP_CLAHE step; false with the reason in *why.
inline bool limits_ok(int clip_q8, int tiles_x, int tiles_y, int mask, int channels, std::string *why) {
  auto fail = [&](const std::string &m) {
    if (why) *why = m;
    return false;
  };
  if (channels != 1 && channels != 3) return fail("channels=" + std::to_string(channels) + ", a frame has 1 or 3");
  if (clip_q8 < 0 || clip_q8 > kMaxClipQ8)
    return fail("clip_q8=" + std::to_string(clip_q8) + " outside 0.." + std::to_string(kMaxClipQ8));
  if (tiles_x < 1 || tiles_x > kMaxTilesAxis)
    return fail("tiles_x=" + std::to_string(tiles_x) + " outside 1.." + std::to_string(kMaxTilesAxis));
  if (tiles_y < 1 || tiles_y > kMaxTilesAxis)
    return fail("tiles_y=" + std::to_string(tiles_y) + " outside 1.." + std::to_string(kMaxTilesAxis));
  if (mask < 0 || mask > 7) return fail("channel mask " + std::to_string(mask) + " outside 0..7");
  if (mask >> channels)
    return fail("channel mask " + std::to_string(mask) + " names a channel beyond the frame's " + std::to_string(channels));
  return true;
}

// A frame of width x height (each at least 1) under the limits: its pixels fit 32 bits and a tile's
// area 31.
inline bool frame_ok(uint64_t width, uint64_t height, int tiles_x, int tiles_y, std::string *why) {
  const uint64_t pixels = width <= kMaxSide && height <= kMaxSide ? width * height : 0;
  if (width > kMaxSide || height > kMaxSide) {
    if (why) *why = "a frame of " + std::to_string(width) + " x " + std::to_string(height) + "; a side is at most " + std::to_string(kMaxSide);
    return false;
  }
  if (pixels > kMaxPixels) {
    if (why) *why = "a frame of " + std::to_string(pixels) + " pixels; at most " + std::to_string(kMaxPixels);
    return false;
  }
  const Geometry g = geometry((uint32_t)width, (uint32_t)height, tiles_x, tiles_y);
  if (g.area > kMaxArea) {
    if (why)
      *why = "a tile of " + std::to_string(g.tw) + " x " + std::to_string(g.th) + " pixels; its area must be at most " +
             std::to_string(kMaxArea);
    return false;
  }
  return true;
}

}  // namespace clahe
}  // namespace vf
