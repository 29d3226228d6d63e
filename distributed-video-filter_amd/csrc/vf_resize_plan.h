// vf_resize_plan.h — what the resize (vf_resize.hip; cv2.resize on 8-bit frames) decides
// outside its loops: the limits of its arguments, the size of the result, the mode a frame resolves to
// (cv2 runs linear at exactly 2 x 2 as area) with its scales, the layout of a VF_STEP_RESIZE step's
// data, the source box of an output tile, and THE RULES: from a destination column or row to the first
// tap and the two 11-bit weights, from a destination index to the nearest source index, and from a
// destination pixel to the mean of its source block.  The rules' text compiles for the host (no HIP
// include is needed: tests/resize/resize_plan_check.cc checks it on the CPU) and for the device, where
// the kernels call the same col_coef, row_coef, nearest_index, linear_pixel and area_pixel.  Every
// float and double operation is one separately rounded IEEE operation: the helpers switch contraction
// off in their own bodies, as vf_clahe_plan.h's and vf_warp_plan.h's do.  Not installed.
#pragma once
#include <stdint.h>

#include <cfloat>
#include <cmath>
#include <string>

#if defined(__HIPCC__)
#define VF_RESIZE_FN __host__ __device__ inline
#else
#define VF_RESIZE_FN inline
#endif
#if defined(__clang__)
#define VF_RESIZE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define VF_RESIZE_NO_CONTRACT
#endif

namespace vf {
namespace resize {

constexpr int kNearest = 0, kLinear = 1, kArea = 3;  // cv2's INTER_NEAREST, INTER_LINEAR, INTER_AREA
constexpr int kMaxSide = 32767;                      // of a source and of a destination
constexpr int kMaxAreaFactor = 16;                   // of an area block, per axis
constexpr int kCoefBits = 11;                        // cv2's INTER_RESIZE_COEF_BITS: the weights sum to 2048
// A VF_STEP_RESIZE step's data: two float64 {fx, fy}, then four int32 {dw, dh, interp, 0}.
constexpr int kStepDoubles = 2, kStepInts = 4;
constexpr size_t kStepBytes = kStepDoubles * sizeof(double) + kStepInts * sizeof(int32_t);

// ---- separately rounded operations ------------------------------------------------------------------------

VF_RESIZE_FN double rounded_mul(double a, double b) {
  VF_RESIZE_NO_CONTRACT
  const double r = a * b;
  return r;
}
VF_RESIZE_FN double rounded_sub(double a, double b) {
  VF_RESIZE_NO_CONTRACT
  const double r = a - b;
  return r;
}
VF_RESIZE_FN float rounded_mulf(float a, float b) {
  VF_RESIZE_NO_CONTRACT
  const float r = a * b;
  return r;
}
VF_RESIZE_FN float rounded_subf(float a, float b) {
  VF_RESIZE_NO_CONTRACT
  const float r = a - b;
  return r;
}

// rint (half to even) and the saturating conversion to int; a NaN gives 0.
VF_RESIZE_FN int round_to_int(double v) {
  const double r = rint(v);
  if (!(r == r)) return 0;
  if (r >= 2147483647.0) return 2147483647;
  if (r <= -2147483648.0) return -2147483647 - 1;
  return (int)r;
}

// ---- a frame's plan ---------------------------------------------------------------------------------------

// What a frame of W x H resolves to: the result's size, the mode after cv2's substitution, the scales
// (source units per destination unit) and, for area, the block's sides.
struct Plan {
  double scale_x, scale_y;
  int32_t W, H, dw, dh;
  int32_t mode;                // kNearest, kLinear or kArea
  int32_t iscale_x, iscale_y;  // area only
};

// The result's size: dsize when both of its sides are non-zero, rint(W fx) x rint(H fy) otherwise.
VF_RESIZE_FN void out_size(int W, int H, int dw, int dh, double fx, double fy, int *ow, int *oh) {
  if (dw != 0 || dh != 0) {
    *ow = dw, *oh = dh;
    return;
  }
  *ow = round_to_int(rounded_mul((double)W, fx));
  *oh = round_to_int(rounded_mul((double)H, fy));
}

// cv2's test for the integer area path, literally: the scale is its own rint to within DBL_EPSILON.
VF_RESIZE_FN bool integer_scale(double scale, int *iscale) {
  *iscale = round_to_int(scale);
  return fabs(rounded_sub(scale, (double)*iscale)) < DBL_EPSILON;
}

// Host: sizes are taken as out_size gives them and must have passed frame_ok.  False: area at a scale
// that is not an integer shrink of at most kMaxAreaFactor (the caller has the message).
inline bool resolve(int W, int H, int dw, int dh, double fx, double fy, int interp, Plan *p) {
  p->W = W, p->H = H;
  if (dw != 0 || dh != 0) {
    const double inv_x = (double)dw / (double)W, inv_y = (double)dh / (double)H;
    p->scale_x = 1.0 / inv_x, p->scale_y = 1.0 / inv_y;
    p->dw = dw, p->dh = dh;
  } else {
    out_size(W, H, 0, 0, fx, fy, &p->dw, &p->dh);
    p->scale_x = 1.0 / fx, p->scale_y = 1.0 / fy;
  }
  int ix = 0, iy = 0;
  const bool fast = integer_scale(p->scale_x, &ix) && integer_scale(p->scale_y, &iy);
  p->iscale_x = ix, p->iscale_y = iy;
  p->mode = interp;
  if (interp == kLinear && fast && ix == 2 && iy == 2) p->mode = kArea;
  if (p->mode == kArea)
    return fast && p->scale_x >= 1.0 && p->scale_y >= 1.0 && ix <= kMaxAreaFactor && iy <= kMaxAreaFactor;
  return true;
}

// ---- the rules --------------------------------------------------------------------------------------------

// nearest: min(floor(d scale), n - 1).
VF_RESIZE_FN int nearest_index(double scale, int d, int n) {
  const double v = floor(rounded_mul((double)d, scale));
  return v >= (double)(n - 1) ? n - 1 : (int)v;
}

// linear: the taps are s and min(s + 1, n - 1) (columns) or clamp(s), clamp(s + 1) (rows).
struct Coef {
  int s, w0, w1;
};

VF_RESIZE_FN int coef_weight(float v) {
  const int w = round_to_int((double)rintf(rounded_mulf(v, 2048.f)));
  return w < -32768 ? -32768 : w > 32767 ? 32767 : w;
}

// f = (float)((d + 0.5) scale - 0.5), s = floor(f), f -= s; columns reset f at both edges, rows do not.
VF_RESIZE_FN Coef axis_coef(double scale, int d, int n, bool edge_reset) {
  float f = (float)rounded_sub(rounded_mul((double)d + 0.5, scale), 0.5);
  const float fl = floorf(f);
  int s = (int)fl;  // |f| < 2^16 under the limits
  f = rounded_subf(f, fl);
  if (edge_reset) {
    if (s < 0) f = 0.f, s = 0;
    if (s >= n - 1) f = 0.f, s = n - 1;
  }
  Coef c;
  c.s = s;
  c.w0 = coef_weight(rounded_subf(1.f, f));
  c.w1 = coef_weight(f);
  return c;
}

VF_RESIZE_FN Coef col_coef(const Plan &p, int dx) { return axis_coef(p.scale_x, dx, p.W, true); }
VF_RESIZE_FN Coef row_coef(const Plan &p, int dy) { return axis_coef(p.scale_y, dy, p.H, false); }

VF_RESIZE_FN int clamp_index(int v, int n) { return v < 0 ? 0 : v > n - 1 ? n - 1 : v; }

// The horizontal pass at one tap row with its >> 4, and the vertical pass: int32, arithmetic shifts.
VF_RESIZE_FN int32_t linear_h(int32_t t0, int32_t t1, int32_t w0, int32_t w1) { return (t0 * w0 + t1 * w1) >> 4; }
VF_RESIZE_FN uint32_t linear_v(int32_t h0, int32_t h1, int32_t b0, int32_t b1) {
  return (uint32_t)((((b0 * h0) >> 16) + ((b1 * h1) >> 16) + 2) >> 2) & 255u;
}

// Channel c of a linear pixel of a frame of packed rows of C interleaved channels.
VF_RESIZE_FN uint32_t linear_pixel(const uint8_t *src, const Plan &p, int C, int c, const Coef &cx, const Coef &cy) {
  const int x0 = cx.s, x1 = cx.s + 1 < p.W ? cx.s + 1 : p.W - 1;
  const uint8_t *r0 = src + (size_t)clamp_index(cy.s, p.H) * (size_t)p.W * (size_t)C + (size_t)c;
  const uint8_t *r1 = src + (size_t)clamp_index(cy.s + 1, p.H) * (size_t)p.W * (size_t)C + (size_t)c;
  return linear_v(linear_h(r0[(size_t)x0 * C], r0[(size_t)x1 * C], cx.w0, cx.w1),
                  linear_h(r1[(size_t)x0 * C], r1[(size_t)x1 * C], cx.w0, cx.w1), cy.w0, cy.w1);
}

VF_RESIZE_FN uint32_t sat_u8_rint(float v) {
  const float r = rintf(v);
  return !(r == r) || r <= 0.f ? 0u : r >= 255.f ? 255u : (uint32_t)r;
}

// area: the mean of the block of iscale_x x iscale_y pixels at (dx iscale_x, dy iscale_y).  A whole
// block: (sum + 2) >> 2 at 2 x 2, the sum times the float 1 / (iscale_x iscale_y) otherwise.  A block
// that overruns the frame (possible only in the fx, fy form) is cv2's slow tail: a column at or past
// W / iscale_x, or any column of a row block that overruns H, takes the pixels inside the frame and
// divides their float sum by their count, whatever the factors.
VF_RESIZE_FN bool area_whole(const Plan &p, int dx, int dy) {
  return dx < p.W / p.iscale_x && dy * p.iscale_y + p.iscale_y <= p.H;
}
VF_RESIZE_FN uint32_t area_mean(const Plan &p, uint32_t sum, uint32_t count, bool whole) {
  if (!whole) return count ? sat_u8_rint((float)sum / (float)count) : 0u;
  if (p.iscale_x == 2 && p.iscale_y == 2) return (sum + 2u) >> 2;
  return sat_u8_rint(rounded_mulf((float)sum, 1.f / (float)(p.iscale_x * p.iscale_y)));
}
VF_RESIZE_FN uint32_t area_pixel(const uint8_t *src, const Plan &p, int C, int c, int dx, int dy) {
  const int sx0 = dx * p.iscale_x, sy0 = dy * p.iscale_y;
  uint32_t sum = 0, count = 0;
  for (int j = 0; j < p.iscale_y && sy0 + j < p.H; ++j) {
    const uint8_t *row = src + ((size_t)(sy0 + j) * (size_t)p.W) * (size_t)C + (size_t)c;
    for (int i = 0; i < p.iscale_x && sx0 + i < p.W; ++i) sum += row[(size_t)(sx0 + i) * C], ++count;
  }
  return area_mean(p, sum, count, area_whole(p, dx, dy));
}

// Channel c of the pixel (dx, dy) under the plan's mode.
VF_RESIZE_FN uint32_t resize_pixel(const uint8_t *src, const Plan &p, int C, int c, int dx, int dy) {
  if (p.mode == kArea) return area_pixel(src, p, C, c, dx, dy);
  if (p.mode == kNearest)
    return src[((size_t)nearest_index(p.scale_y, dy, p.H) * (size_t)p.W + (size_t)nearest_index(p.scale_x, dx, p.W)) * (size_t)C +
               (size_t)c];
  return linear_pixel(src, p, C, c, col_coef(p, dx), row_coef(p, dy));
}

// ---- the step's data -------------------------------------------------------------------------------------

struct StepData {
  double fx, fy;
  int dw, dh, interp;
};

// ---- an output tile's source box --------------------------------------------------------------------------

// The pixels that output columns [x0, x1] and rows [y0, y1] (inclusive) read lie in columns
// [sx_lo, sx_hi] and rows [sy_lo, sy_hi] of the frame, after every clamp.  The first tap is monotone in
// the destination index (a product with a positive constant, a difference with a constant, the
// conversion to float, floor, and the clamps are each monotone), so the box of an axis runs from the
// first index's first tap to the last index's last tap; it is exact.
struct Box {
  int sx_lo, sx_hi, sy_lo, sy_hi;
};

VF_RESIZE_FN Box tile_footprint(const Plan &p, int x0, int x1, int y0, int y1) {
  Box b;
  if (p.mode == kArea) {
    b.sx_lo = x0 * p.iscale_x, b.sx_hi = clamp_index(x1 * p.iscale_x + p.iscale_x - 1, p.W);
    b.sy_lo = y0 * p.iscale_y, b.sy_hi = clamp_index(y1 * p.iscale_y + p.iscale_y - 1, p.H);
  } else if (p.mode == kNearest) {
    b.sx_lo = nearest_index(p.scale_x, x0, p.W), b.sx_hi = nearest_index(p.scale_x, x1, p.W);
    b.sy_lo = nearest_index(p.scale_y, y0, p.H), b.sy_hi = nearest_index(p.scale_y, y1, p.H);
  } else {
    b.sx_lo = col_coef(p, x0).s, b.sx_hi = clamp_index(col_coef(p, x1).s + 1, p.W);
    b.sy_lo = clamp_index(row_coef(p, y0).s, p.H), b.sy_hi = clamp_index(row_coef(p, y1).s + 1, p.H);
  }
  return b;
}

// ---- limits (host) ----------------------------------------------------------------------------------------

// The filter arguments of every entry point and of a VF_STEP_RESIZE step; false with the reason in *why.
inline bool limits_ok(int dw, int dh, double fx, double fy, int interp, int channels, std::string *why) {
  auto fail = [&](const std::string &s) {
    if (why) *why = s;
    return false;
  };
  if (channels != 1 && channels != 3) return fail("channels=" + std::to_string(channels) + ", a frame has 1 or 3");
  if (interp == 2 || interp == 4)
    return fail("interpolation " + std::to_string(interp) + " (cubic, Lanczos) is not built; nearest 0, linear 1 and area 3 are");
  if (interp != kNearest && interp != kLinear && interp != kArea)
    return fail("unknown interpolation " + std::to_string(interp) + "; nearest 0, linear 1 and area 3 are built");
  if (dw < 0 || dh < 0 || dw > kMaxSide || dh > kMaxSide)
    return fail("dsize " + std::to_string(dw) + " x " + std::to_string(dh) + "; a side is 1 to " + std::to_string(kMaxSide));
  if ((dw == 0) != (dh == 0))
    return fail("dsize " + std::to_string(dw) + " x " + std::to_string(dh) + " has a side of 0");
  if (dw == 0 && !(std::isfinite(fx) && std::isfinite(fy) && fx > 0.0 && fy > 0.0))
    return fail("without dsize, fx and fy are finite and positive (fx=" + std::to_string(fx) + ", fy=" + std::to_string(fy) + ")");
  return true;
}

// A frame of width x height (each at least 1) under the arguments: both sizes within the limits, and
// the plan in *p (which may be NULL).
inline bool frame_ok(uint64_t width, uint64_t height, int dw, int dh, double fx, double fy, int interp, Plan *p,
                     std::string *why) {
  auto fail = [&](const std::string &s) {
    if (why) *why = s;
    return false;
  };
  if (width > (uint64_t)kMaxSide || height > (uint64_t)kMaxSide)
    return fail("a frame of " + std::to_string(width) + " x " + std::to_string(height) + "; a side is at most " +
                std::to_string(kMaxSide));
  int ow = 0, oh = 0;
  out_size((int)width, (int)height, dw, dh, fx, fy, &ow, &oh);
  if (ow < 1 || oh < 1)
    return fail("a frame of " + std::to_string(width) + " x " + std::to_string(height) + " resizes to " + std::to_string(ow) +
                " x " + std::to_string(oh) + ": a side of 0");
  if (ow > kMaxSide || oh > kMaxSide)
    return fail("a frame of " + std::to_string(width) + " x " + std::to_string(height) + " resizes to " + std::to_string(ow) +
                " x " + std::to_string(oh) + "; a side is at most " + std::to_string(kMaxSide));
  Plan q;
  if (!resolve((int)width, (int)height, dw, dh, fx, fy, interp, &q))
    return fail("area from " + std::to_string(width) + " x " + std::to_string(height) + " to " + std::to_string(ow) + " x " +
                std::to_string(oh) + ": area is built for integer shrink factors of 1 to " + std::to_string(kMaxAreaFactor) +
                " on both axes only");
  if (p) *p = q;
  return true;
}

}  // namespace resize
}  // namespace vf
