// resize_plan_check.cc — the rules and the limits of csrc/vf_resize_plan.h on the CPU (tests/test_resize_plan.py
// builds this with -fsanitize=address,undefined -ffp-contract=off and runs it as a program).
//
//   axis       stdin lines "n_src n_dst": per line, for every destination index of the dsize form,
//              col_coef's s w0 w1, row_coef's s w0 w1 and nearest_index
//   pixels     stdin lines "W H C dw dh fx fy interp hex-bytes-of-the-frame" (the doubles as their 64-bit
//              patterns, decimal): "dw dh" and the resized frame's bytes through frame_ok and resize_pixel,
//              or "refused" and nothing else
//   footprint  tile_footprint against every pixel of every tile, on frames up to 40 x 40 and destinations up
//              to 60 x 60 under the three modes and both forms: {"checked", "failed"}
//   limits     limits_ok and frame_ok, what they accept and the reasons they give: {"checked", "failed"}
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "vf_resize_plan.h"

namespace Z = vf::resize;

static double from_bits(uint64_t b) {
  double d;
  std::memcpy(&d, &b, sizeof d);
  return d;
}

static int axis() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    int n, d;
    if (!(in >> n >> d)) return 2;
    Z::Plan p;
    if (!Z::frame_ok((uint64_t)n, (uint64_t)n, d, d, 0, 0, Z::kNearest, &p, nullptr)) return 3;
    for (int i = 0; i < d; ++i) {
      const Z::Coef c = Z::col_coef(p, i), r = Z::row_coef(p, i);
      std::printf("%d %d %d %d %d %d %d ", c.s, c.w0, c.w1, r.s, r.w0, r.w1, Z::nearest_index(p.scale_x, i, n));
    }
    std::printf("\n");
  }
  return 0;
}

static int pixels() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    int w, h, c, dw, dh, interp;
    uint64_t bx, by;
    std::string hex;
    if (!(in >> w >> h >> c >> dw >> dh >> bx >> by >> interp >> hex)) return 2;
    if (hex.size() != (size_t)w * h * c * 2) return 2;
    std::vector<uint8_t> src((size_t)w * h * c);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)std::stoi(hex.substr(2 * i, 2), nullptr, 16);
    Z::Plan p;
    std::string why;
    if (!Z::limits_ok(dw, dh, from_bits(bx), from_bits(by), interp, c, &why) ||
        !Z::frame_ok((uint64_t)w, (uint64_t)h, dw, dh, from_bits(bx), from_bits(by), interp, &p, &why)) {
      std::printf("refused\n");
      continue;
    }
    std::printf("%d %d ", p.dw, p.dh);
    for (int y = 0; y < p.dh; ++y)
      for (int x = 0; x < p.dw; ++x)
        for (int k = 0; k < c; ++k) std::printf("%u ", Z::resize_pixel(src.data(), p, c, k, x, y));
    std::printf("\n");
  }
  return 0;
}

// The pixels one destination pixel reads, after every clamp, as a box of its own.
static Z::Box reads(const Z::Plan &p, int x, int y) {
  Z::Box b;
  if (p.mode == Z::kArea) {
    b.sx_lo = x * p.iscale_x, b.sy_lo = y * p.iscale_y;
    b.sx_hi = std::min(b.sx_lo + p.iscale_x, (int)p.W) - 1, b.sy_hi = std::min(b.sy_lo + p.iscale_y, (int)p.H) - 1;
  } else if (p.mode == Z::kNearest) {
    b.sx_lo = b.sx_hi = Z::nearest_index(p.scale_x, x, p.W);
    b.sy_lo = b.sy_hi = Z::nearest_index(p.scale_y, y, p.H);
  } else {
    const Z::Coef cx = Z::col_coef(p, x), cy = Z::row_coef(p, y);
    b.sx_lo = cx.s, b.sx_hi = std::min(cx.s + 1, p.W - 1);
    b.sy_lo = Z::clamp_index(cy.s, p.H), b.sy_hi = Z::clamp_index(cy.s + 1, p.H);
  }
  return b;
}

static int footprint() {
  long checked = 0, failed = 0;
  const int sizes[][2] = {{1, 1}, {2, 2}, {5, 3}, {9, 1}, {1, 9}, {17, 11}, {40, 40}, {39, 23}, {32, 16}};
  const int dsts[][2] = {{1, 1}, {5, 3}, {4, 1}, {1, 20}, {7, 5}, {60, 60}, {59, 37}, {16, 8}, {13, 23}, {20, 20}, {8, 4}};
  const double fs[] = {0.5, 0.25, 0.3, 1.0, 1.5, 1.0 / 3.0};
  const int tiles[][2] = {{64, 16}, {7, 3}, {1, 1}, {16, 5}};
  for (const auto &s : sizes)
    for (int interp : {Z::kNearest, Z::kLinear, Z::kArea})
      for (int form = 0; form < 2; ++form)
        for (size_t k = 0; k < (form ? sizeof fs / sizeof *fs : sizeof dsts / sizeof *dsts); ++k) {
          Z::Plan p;
          if (!Z::frame_ok((uint64_t)s[0], (uint64_t)s[1], form ? 0 : dsts[k][0], form ? 0 : dsts[k][1], form ? fs[k] : 0,
                           form ? fs[k] : 0, interp, &p, nullptr))
            continue;
          for (const auto &t : tiles)
            for (int y0 = 0; y0 < p.dh; y0 += t[1])
              for (int x0 = 0; x0 < p.dw; x0 += t[0]) {
                const int x1 = std::min(x0 + t[0], (int)p.dw) - 1, y1 = std::min(y0 + t[1], (int)p.dh) - 1;
                Z::Box want = {1 << 30, -1, 1 << 30, -1};
                for (int y = y0; y <= y1; ++y)
                  for (int x = x0; x <= x1; ++x) {
                    const Z::Box r = reads(p, x, y);
                    want.sx_lo = std::min(want.sx_lo, r.sx_lo), want.sx_hi = std::max(want.sx_hi, r.sx_hi);
                    want.sy_lo = std::min(want.sy_lo, r.sy_lo), want.sy_hi = std::max(want.sy_hi, r.sy_hi);
                  }
                const Z::Box got = Z::tile_footprint(p, x0, x1, y0, y1);
                ++checked;
                const bool ok = got.sx_lo == want.sx_lo && got.sx_hi == want.sx_hi && got.sy_lo == want.sy_lo &&
                                got.sy_hi == want.sy_hi && got.sx_lo >= 0 && got.sy_lo >= 0 && got.sx_hi < p.W && got.sy_hi < p.H;
                if (!ok && ++failed <= 5)
                  std::fprintf(stderr, "footprint %dx%d -> %dx%d mode %d tile (%d..%d, %d..%d): got %d..%d %d..%d want %d..%d %d..%d\n",
                               p.W, p.H, p.dw, p.dh, p.mode, x0, x1, y0, y1, got.sx_lo, got.sx_hi, got.sy_lo, got.sy_hi, want.sx_lo,
                               want.sx_hi, want.sy_lo, want.sy_hi);
              }
        }
  std::printf("{\"checked\": %ld, \"failed\": %ld}\n", checked, failed);
  return failed ? 1 : 0;
}

static long g_checked = 0, g_failed = 0;
static void expect(bool ok, const char *what) {
  ++g_checked;
  if (!ok && ++g_failed <= 10) std::fprintf(stderr, "limits: %s\n", what);
}
static bool has(const std::string &s, const char *part) { return s.find(part) != std::string::npos; }

static int limits() {
  std::string why;
  expect(Z::limits_ok(10, 10, 0, 0, Z::kLinear, 3, &why), "a dsize");
  expect(Z::limits_ok(0, 0, 0.5, 2.0, Z::kArea, 1, &why), "fx and fy");
  expect(Z::limits_ok(32767, 1, 0, 0, Z::kNearest, 1, &why), "the largest side");
  expect(!Z::limits_ok(10, 10, 0, 0, Z::kLinear, 2, &why) && has(why, "channels=2"), "two channels");
  expect(!Z::limits_ok(10, 10, 0, 0, 2, 3, &why) && has(why, "not built"), "cubic");
  expect(!Z::limits_ok(10, 10, 0, 0, 4, 3, &why) && has(why, "not built"), "Lanczos");
  expect(!Z::limits_ok(10, 10, 0, 0, 5, 3, &why) && has(why, "unknown interpolation 5"), "interp 5");
  expect(!Z::limits_ok(10, 10, 0, 0, -1, 3, &why) && has(why, "unknown interpolation -1"), "interp -1");
  expect(!Z::limits_ok(32768, 10, 0, 0, Z::kLinear, 3, &why) && has(why, "a side is 1 to 32767"), "a side of 32768");
  expect(!Z::limits_ok(-1, 10, 0, 0, Z::kLinear, 3, &why) && has(why, "a side is 1 to 32767"), "a negative side");
  expect(!Z::limits_ok(10, 0, 0, 0, Z::kLinear, 3, &why) && has(why, "has a side of 0"), "one side of 0");
  expect(!Z::limits_ok(0, 0, 0, 0.5, Z::kLinear, 3, &why) && has(why, "finite and positive"), "fx of 0");
  expect(!Z::limits_ok(0, 0, 0.5, -1, Z::kLinear, 3, &why) && has(why, "finite and positive"), "a negative fy");
  expect(!Z::limits_ok(0, 0, NAN, 1, Z::kLinear, 3, &why) && has(why, "finite and positive"), "a NaN");
  expect(!Z::limits_ok(0, 0, INFINITY, 1, Z::kLinear, 3, &why) && has(why, "finite and positive"), "an infinity");

  Z::Plan p;
  expect(Z::frame_ok(12, 12, 6, 6, 0, 0, Z::kLinear, &p, &why) && p.mode == Z::kArea && p.iscale_x == 2, "linear at 2 x 2 is area");
  expect(Z::frame_ok(12, 12, 6, 4, 0, 0, Z::kLinear, &p, &why) && p.mode == Z::kLinear, "linear at 2 x 3 stays");
  expect(Z::frame_ok(12, 12, 0, 0, 0.5, 0.5, Z::kLinear, &p, &why) && p.mode == Z::kArea && p.dw == 6, "the fx form at 2 x 2");
  expect(Z::frame_ok(5, 7, 0, 0, 0.5, 0.5, Z::kNearest, &p, &why) && p.dw == 2 && p.dh == 4, "half to even");
  expect(p.scale_x == 2.0 && p.scale_y == 2.0, "the fx form's scale is 1 / fx");
  expect(Z::frame_ok(300, 80, 20, 5, 0, 0, Z::kArea, &p, &why) && p.iscale_x == 15 && p.iscale_y == 16, "area 15 x 16");
  expect(Z::frame_ok(12, 12, 12, 12, 0, 0, Z::kArea, &p, &why) && p.iscale_x == 1, "area 1 x 1");
  expect(!Z::frame_ok(12, 12, 8, 8, 0, 0, Z::kArea, &p, &why) && has(why, "integer shrink factors"), "area at 1.5");
  expect(!Z::frame_ok(12, 12, 24, 12, 0, 0, Z::kArea, &p, &why) && has(why, "integer shrink factors"), "area as an upscale");
  expect(!Z::frame_ok(34, 34, 2, 2, 0, 0, Z::kArea, &p, &why) && has(why, "integer shrink factors"), "area 17 x 17");
  expect(!Z::frame_ok(32768, 2, 2, 2, 0, 0, Z::kLinear, &p, &why) && has(why, "a side is at most 32767"), "a source side of 32768");
  expect(!Z::frame_ok(3, 3, 0, 0, 0.1, 0.1, Z::kLinear, &p, &why) && has(why, "a side of 0"), "a result side of 0");
  expect(!Z::frame_ok(30000, 3, 0, 0, 2.0, 1.0, Z::kLinear, &p, &why) && has(why, "a side is at most 32767"), "a result side of 60000");
  expect(!Z::frame_ok(30000, 3, 0, 0, 1e300, 1.0, Z::kLinear, &p, &why) && has(why, "a side is at most 32767"), "a saturated side");
  std::printf("{\"checked\": %ld, \"failed\": %ld}\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "axis") return axis();
  if (mode == "pixels") return pixels();
  if (mode == "footprint") return footprint();
  if (mode == "limits") return limits();
  std::fprintf(stderr, "usage: resize_plan_check axis|pixels|footprint|limits\n");
  return 2;
}
