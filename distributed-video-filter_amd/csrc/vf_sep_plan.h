// vf_sep_plan.h — what the separable filter (vf_sep.hip; cv2.sepFilter2D, cv2.blur, cv2.boxFilter;
// DESIGN.md 21) decides on the host (host only, no HIP, so tests/sep/sep_plan_check.cc checks it on
// the CPU): the limits of its arguments, the tile geometry its launcher picks for a (kw, kh), and
// the exact divisions by a constant its kernel uses.  Not installed.
#pragma once
#include <stdint.h>

#include <cstdlib>
#include <string>

#include "vf_conv_border.h"

namespace vf {
namespace sep {

constexpr int kMaxSide = 31;               // taps per axis: odd, 1 .. 31
constexpr int kMaxTaps = 2 * kMaxSide;     // both axes
constexpr long kMaxSum = 65536;            // sum|kx| * sum|ky|
constexpr int kMaxShift = 16;
constexpr int kMaxDivisor = 1023;          // odd; 1: none
constexpr int kRoundHalfEven = 0, kRoundHalfUp = 1;  // VF_ROUND_*

constexpr int kTileBytes = 256;            // row bytes of a workgroup's output tile
constexpr int kMaxLds = 64 * 1024;         // the LDS a workgroup may ask for without opting in

inline long abs_sum(const int16_t *k, int n) {
  long s = 0;
  for (int i = 0; i < n; ++i) s += std::labs((long)k[i]);
  return s;
}

inline bool side_ok(int n) { return n >= 1 && n <= kMaxSide && (n & 1); }

// The filter arguments of every entry point; false with the reason in *why.
inline bool limits_ok(const int16_t *kx, int kw, const int16_t *ky, int kh, int shift, int divisor, int rounding,
                      int border, std::string *why) {
  auto fail = [&](const std::string &m) {
    if (why) *why = m;
    return false;
  };
  if (!kx || !ky) return fail("taps are NULL");
  if (!side_ok(kw) || !side_ok(kh))
    return fail("a " + std::to_string(kw) + " x " + std::to_string(kh) + " separable kernel; tap counts are odd and at most " +
                std::to_string(kMaxSide));
  const long sx = abs_sum(kx, kw), sy = abs_sum(ky, kh);
  if (sx * sy > kMaxSum)
    return fail("sum|kx| * sum|ky| = " + std::to_string(sx * sy) + " exceeds " + std::to_string(kMaxSum));
  if (shift < 0 || shift > kMaxShift) return fail("shift=" + std::to_string(shift) + " outside 0..16");
  if (divisor < 1 || divisor > kMaxDivisor || !(divisor & 1))
    return fail("divisor=" + std::to_string(divisor) + "; a divisor is odd and 1 .. " + std::to_string(kMaxDivisor));
  if (shift != 0 && divisor != 1)
    return fail("shift=" + std::to_string(shift) + " together with divisor=" + std::to_string(divisor) +
                "; a filter scales by one of them");
  if (rounding != kRoundHalfEven && rounding != kRoundHalfUp) return fail("unknown rounding " + std::to_string(rounding));
  if (border != conv::kReflect101 && border != conv::kReplicate && border != conv::kConstant)
    return fail("unknown border " + std::to_string(border));
  return true;
}

// ---- geometry --------------------------------------------------------------------------------------
// The vertical pass runs first: a workgroup stages (rows + 2 ry) x stage_bytes source bytes, the
// vertical pass leaves rows x stage_bytes wide sums, the horizontal pass rows x kTileBytes results.

// Is the vertical pass's sum a 16-bit value?  |sum| <= 255 * sum|ky|.
inline bool narrow_fits(const int16_t *ky, int kh) { return 255 * abs_sum(ky, kh) < 32768; }

struct Geometry {
  int rows;         // output rows of a tile
  int halo;         // staged bytes on either side of the tile's kTileBytes: a 16-B multiple >= (kw / 2) * C
  int stage_rows;   // rows + 2 * (kh / 2)
  int stage_bytes;  // kTileBytes + 2 * halo: the LDS row pitch of the staged bytes and of the sums
  int elem_bytes;   // of a vertical sum: 2 or 4
  int lds_bytes;    // stage_rows * stage_bytes + rows * stage_bytes * elem_bytes
};

// The rows of a tile for kh vertical taps (vf_sep_tile reports it): 16 for every kh, as measured on
// 1080p x 32 (profiles/sep_raw_bench.txt).  A taller tile re-reads less halo but its
// LDS leaves fewer workgroups a CU: at 31 taps 24 rows take 1.10 to 1.19 x the time of 16, and at 7
// taps they take 0.95 x with 16-bit sums but 1.22 x with 32-bit sums.
inline int tile_rows(int kh) { return kh >= 1 ? 16 : 0; }

inline Geometry geometry(int kw, int kh, int channels, bool narrow, int rows) {
  Geometry g;
  g.rows = rows;
  g.halo = ((kw / 2) * channels + 15) / 16 * 16;
  g.stage_rows = rows + 2 * (kh / 2);
  g.stage_bytes = kTileBytes + 2 * g.halo;
  g.elem_bytes = narrow ? 2 : 4;
  g.lds_bytes = g.stage_rows * g.stage_bytes + rows * g.stage_bytes * g.elem_bytes;
  return g;
}

inline bool rows_ok(int rows) { return rows >= 16 && rows <= 32 && rows % 8 == 0; }

// ---- exact divisions ---------------------------------------------------------------------------------

// floor(x / n) as the high word of x * recip(n): exact while x * n < 2^32 (the kernel splits a
// staging item, below 62 * 22, by the 16-B pieces of a staged row, at most 22)
inline uint32_t recip(uint32_t n) { return (uint32_t)(((uint64_t)1 << 32) / n) + 1; }
inline uint32_t div_recip(uint32_t x, uint32_t r) { return (uint32_t)(((uint64_t)x * r) >> 32); }

// The divisor d (odd, 1 .. 1023): q = floor((2 acc + d) / (2 d)) clamped to 0 .. 255, to nearest
// without ties.  acc is clamped to [0, top] first (below it the result is 0, above it 255), so
// N = 2 acc + d < 2^20 and q = (N * mul) >> 40 in 64 bits.
struct Divide {
  int32_t d, top;
  uint64_t mul;
};
inline Divide divide_by(int d) {
  Divide v;
  v.d = d;
  v.top = 255 * d + (d - 1) / 2;
  v.mul = (((uint64_t)1 << 40) / (uint64_t)(2 * d)) + 1;
  return v;
}
inline int divide(const Divide &v, int acc) {
  const int c = acc < 0 ? 0 : acc > v.top ? v.top : acc;
  return (int)(((uint64_t)(uint32_t)(2 * c + v.d) * v.mul) >> 40);
}

}  // namespace sep
}  // namespace vf
