// vf_warp_plan.h — what the affine warp (vf_warp.hip; cv2.warpAffine and cv2.flip on 8-bit frames;
// DESIGN.md 24) decides outside its loops: the limits of its arguments, the map a flip resolves to
// for a frame, the layout of a VF_STEP_WARP step's data, the source box of an output tile, and THE
// RULES: from a column and a row to the fixed-point source coordinate, from the coordinate to the
// tap position and the four weights, from a tap position to the frame's index under a border, and
// from the taps to the pixel.  The rules' text compiles for the host (no HIP include is needed:
// tests/warp/warp_plan_check.cc checks it on the CPU, built with -ffp-contract=off) and for the
// device, where the kernels call the same col_delta, row_base, warp_coord, warp_weights, border_at
// and warp_pixel.  Every double operation is one separately rounded IEEE operation: nothing is fused
// (rounded_mul, rounded_add).  Not installed.
#pragma once
#include <stdint.h>

#include <cmath>
#include <string>

#include "vf_conv_border.h"

#if defined(__HIPCC__)
#define VF_WARP_FN __host__ __device__ inline
#else
#define VF_WARP_FN inline
#endif
// As vf_clahe_plan.h's: a product whose result feeds a sum must not become a fused multiply-add, so
// each operation is a function of its own with contraction switched off in its body.
#if defined(__clang__)
#define VF_WARP_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define VF_WARP_NO_CONTRACT
#endif

namespace vf {
namespace warp {

VF_WARP_FN double rounded_mul(double a, double b) {
  VF_WARP_NO_CONTRACT
  const double r = a * b;
  return r;
}
VF_WARP_FN double rounded_add(double a, double b) {
  VF_WARP_NO_CONTRACT
  const double r = a + b;
  return r;
}

constexpr int kLinear = 0, kNearest = 1;                             // interp
constexpr int kAffine = 0, kFlipH = 1, kFlipV = 2, kFlipBoth = 3;    // mode
constexpr int kAbBits = 10, kInterBits = 5;                          // cv2's AB_BITS and INTER_BITS
constexpr int kMaxSide = 32767;                                      // of a frame: a tap index fits 16 bits and one more
constexpr double kCoordLimit = 1073741824.0;                         // 2^30: every fixed-point term stays below it
// A VF_STEP_WARP step's data: six float64 (m), then six int32 {mode, interp, value B, G, R, 0}.
constexpr int kStepDoubles = 6, kStepInts = 6;
constexpr size_t kStepBytes = kStepDoubles * sizeof(double) + kStepInts * sizeof(int32_t);

// ---- the map ---------------------------------------------------------------------------------------------

// The map of a frame of W x H: the given m, or the flip's.
VF_WARP_FN void resolve(int mode, const double *m, int W, int H, double *out) {
  if (mode == kAffine) {
    for (int i = 0; i < 6; ++i) out[i] = m[i];
    return;
  }
  const bool fx = mode == kFlipH || mode == kFlipBoth, fy = mode == kFlipV || mode == kFlipBoth;
  out[0] = fx ? -1.0 : 1.0, out[1] = 0.0, out[2] = fx ? (double)(W - 1) : 0.0;
  out[3] = 0.0, out[4] = fy ? -1.0 : 1.0, out[5] = fy ? (double)(H - 1) : 0.0;
}

// ---- the coordinate rule ---------------------------------------------------------------------------------

// rint (half to even) and the saturating conversion to int; a NaN gives 0.
VF_WARP_FN int round_to_int(double v) {
  const double r = rint(v);
  if (!(r == r)) return 0;
  if (r >= 2147483647.0) return 2147483647;
  if (r <= -2147483648.0) return -2147483647 - 1;
  return (int)r;
}

// adelta(x) = int(rint((m0 x) 1024)) with mk = m0, bdelta(x) with mk = m3.
VF_WARP_FN int col_delta(double mk, int x) { return round_to_int(rounded_mul(rounded_mul(mk, (double)x), 1024.0)); }

// X0(y) = int(rint((m1 y + m2) 1024)) + rd with (ma, mb) = (m1, m2), Y0(y) with (m4, m5); rd: round_delta.
VF_WARP_FN int round_delta(int interp) { return interp == kNearest ? 512 : 16; }
VF_WARP_FN int row_base(double ma, double mb, int y, int rd) {
  const int v = round_to_int(rounded_mul(rounded_add(rounded_mul(ma, (double)y), mb), 1024.0));
  return (int)((uint32_t)v + (uint32_t)rd);  // no overflow under the limits; never undefined
}

VF_WARP_FN int clamp_short(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

// One axis of a pixel: the first tap's position and, for linear, the fraction in 1 / 32.
struct Coord {
  int s, f;
};

// base: row_base of the pixel's row; delta: col_delta of its column.  Arithmetic shifts.
VF_WARP_FN Coord warp_coord(int base, int delta, int interp) {
  const int sum = (int)((uint32_t)base + (uint32_t)delta);
  Coord c;
  if (interp == kNearest) {
    c.s = clamp_short(sum >> kAbBits);
    c.f = 0;
  } else {
    const int v = sum >> (kAbBits - kInterBits);
    c.s = clamp_short(v >> kInterBits);
    c.f = v & ((1 << kInterBits) - 1);
  }
  return c;
}

// The four taps' weights, (sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1): they sum to 32768.
struct Weights {
  uint32_t w00, w01, w10, w11;
};

VF_WARP_FN Weights warp_weights(int fx, int fy) {
  Weights w;
  w.w00 = 32u * (uint32_t)(32 - fx) * (uint32_t)(32 - fy);
  w.w01 = 32u * (uint32_t)fx * (uint32_t)(32 - fy);
  w.w10 = 32u * (uint32_t)(32 - fx) * (uint32_t)fy;
  w.w11 = 32u * (uint32_t)fx * (uint32_t)fy;
  return w;
}

VF_WARP_FN uint32_t warp_blend(uint32_t t00, uint32_t t01, uint32_t t10, uint32_t t11, const Weights &w) {
  return (w.w00 * t00 + w.w01 * t01 + w.w10 * t10 + w.w11 * t11 + 16384u) >> 15;
}

// ---- the border ------------------------------------------------------------------------------------------

// conv::border_index in closed form: the index on an axis of n >= 1 elements that position p reads,
// -1 for the constant border outside the axis.  Reflect-101 is a triangle wave of period 2 n - 2, so
// a saturated coordinate of -32768 on a 2-element axis is one remainder, not sixteen thousand turns.
VF_WARP_FN int border_at(int p, int n, int border) {
  if (p >= 0 && p < n) return p;
  if (border == conv::kConstant) return -1;
  if (border == conv::kReplicate) return p < 0 ? 0 : n - 1;
  if (n == 1) return 0;
  const int period = 2 * n - 2;
  int q = p % period;
  if (q < 0) q += period;
  return q < n ? q : period - q;
}

// ---- the pixel -------------------------------------------------------------------------------------------

// The tap at (ty, tx) of channel c of a frame of W x H pixels of C interleaved channels, packed rows.
VF_WARP_FN uint32_t warp_tap(const uint8_t *src, int W, int H, int C, int c, int ty, int tx, int border, uint32_t value) {
  const int iy = border_at(ty, H, border), ix = border_at(tx, W, border);
  if (iy < 0 || ix < 0) return value;
  return src[((size_t)iy * (size_t)W + (size_t)ix) * (size_t)C + (size_t)c];
}

// Channel c of the pixel whose axes' coordinates are cx and cy.  value: the constant border's byte.
VF_WARP_FN uint32_t warp_pixel(const uint8_t *src, int W, int H, int C, int c, Coord cx, Coord cy, int interp, int border,
                               uint32_t value) {
  if (interp == kNearest) return warp_tap(src, W, H, C, c, cy.s, cx.s, border, value);
  const Weights w = warp_weights(cx.f, cy.f);
  return warp_blend(warp_tap(src, W, H, C, c, cy.s, cx.s, border, value), warp_tap(src, W, H, C, c, cy.s, cx.s + 1, border, value),
                    warp_tap(src, W, H, C, c, cy.s + 1, cx.s, border, value),
                    warp_tap(src, W, H, C, c, cy.s + 1, cx.s + 1, border, value), w);
}

// ---- an output tile's source box -------------------------------------------------------------------------

// The taps of output columns [x0, x1] and rows [y0, y1] (inclusive, x0 <= x1, y0 <= y1) lie in
// columns [sx_lo, sx_hi] and rows [sy_lo, sy_hi], before any border rule.  adelta and bdelta are
// monotone in x, X0 and Y0 in y (a product with a constant, a sum with a constant and rint are each
// monotone), and so are the sum, the shift and the clamp: every first tap of the tile lies between
// the values at its four corners.  Linear adds one for the second tap.
struct Box {
  int sx_lo, sx_hi, sy_lo, sy_hi;
};

VF_WARP_FN Box tile_footprint(const double *m, int interp, int x0, int x1, int y0, int y1) {
  const int rd = round_delta(interp);
  Box b = {2147483647, -2147483647 - 1, 2147483647, -2147483647 - 1};
  for (int k = 0; k < 4; ++k) {
    const int x = k & 1 ? x1 : x0, y = k & 2 ? y1 : y0;
    const int sx = warp_coord(row_base(m[1], m[2], y, rd), col_delta(m[0], x), interp).s;
    const int sy = warp_coord(row_base(m[4], m[5], y, rd), col_delta(m[3], x), interp).s;
    b.sx_lo = sx < b.sx_lo ? sx : b.sx_lo, b.sx_hi = sx > b.sx_hi ? sx : b.sx_hi;
    b.sy_lo = sy < b.sy_lo ? sy : b.sy_lo, b.sy_hi = sy > b.sy_hi ? sy : b.sy_hi;
  }
  if (interp == kLinear) ++b.sx_hi, ++b.sy_hi;
  return b;
}

// ---- the step's data -------------------------------------------------------------------------------------

struct StepData {
  double m[6];
  int mode, interp;
  uint8_t value[3];
};

// ---- limits (host) ---------------------------------------------------------------------------------------

// The filter arguments of every entry point and of a VF_STEP_WARP step; false with the reason in *why.
// value: the three ints of the border colour.
inline bool limits_ok(const double *m, int mode, int interp, int border, const int *value, int channels, std::string *why) {
  auto fail = [&](const std::string &s) {
    if (why) *why = s;
    return false;
  };
  if (channels != 1 && channels != 3) return fail("channels=" + std::to_string(channels) + ", a frame has 1 or 3");
  if (mode < kAffine || mode > kFlipBoth) return fail("mode=" + std::to_string(mode) + " outside 0..3");
  if (interp != kLinear && interp != kNearest) return fail("interp=" + std::to_string(interp) + " outside 0..1");
  if (border != conv::kReflect101 && border != conv::kReplicate && border != conv::kConstant)
    return fail("unknown border " + std::to_string(border));
  if (!value) return fail("value is NULL");
  for (int c = 0; c < 3; ++c)
    if (value[c] < 0 || value[c] > 255) return fail("value[" + std::to_string(c) + "]=" + std::to_string(value[c]) + " outside 0..255");
  if (mode == kAffine) {
    if (!m) return fail("m is NULL");
    for (int i = 0; i < 6; ++i)
      if (!std::isfinite(m[i])) return fail("m[" + std::to_string(i) + "] is not finite");
  }
  return true;
}

// A frame of width x height (each at least 1) under the map's limits: sides of at most 32767, and
// every fixed-point term below 2^30, so no conversion saturates and no int sum overflows.
inline bool frame_ok(uint64_t width, uint64_t height, int mode, const double *m, std::string *why) {
  auto fail = [&](const std::string &s) {
    if (why) *why = s;
    return false;
  };
  if (width > (uint64_t)kMaxSide || height > (uint64_t)kMaxSide)
    return fail("a frame of " + std::to_string(width) + " x " + std::to_string(height) + "; a side is at most " +
                std::to_string(kMaxSide));
  double r[6];
  resolve(mode, m, (int)width, (int)height, r);
  const double xs = (double)(width - 1), ys = (double)(height - 1);
  for (int axis = 0; axis < 2; ++axis) {
    const int k = 3 * axis;
    const std::string mk = "m[" + std::to_string(k) + "]", ma = "m[" + std::to_string(k + 1) + "]", mb = "m[" + std::to_string(k + 2) + "]";
    if (!(std::fabs(r[k]) * xs * 1024.0 < kCoordLimit))
      return fail(mk + "=" + std::to_string(r[k]) + " over " + std::to_string(width) + " columns leaves the fixed-point range (2^30 / 1024)");
    for (int e = 0; e < 2; ++e) {
      const double y = e ? ys : 0.0;
      if (!(std::fabs(r[k + 1] * y + r[k + 2]) * 1024.0 + 512.0 < kCoordLimit))
        return fail(ma + "=" + std::to_string(r[k + 1]) + " and " + mb + "=" + std::to_string(r[k + 2]) + " at row " +
                    std::to_string((uint64_t)y) + " leave the fixed-point range (2^30 / 1024)");
    }
  }
  return true;
}

}  // namespace warp
}  // namespace vf
