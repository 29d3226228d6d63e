// warp_plan_check.cc — the rules and the limits of csrc/vf_warp_plan.h on the CPU (tests/test_warp_plan.py
// builds this with -fsanitize=address,undefined -ffp-contract=off and runs it as a program).
//
//   coords     stdin lines "W H interp m0 .. m5" (the doubles as their 64-bit patterns, decimal): per line
//              sx sy fx fy of every pixel, row by row, through col_delta, row_base and warp_coord
//   weights    the four weights of every (fx, fy), fy outermost: one line
//   border_at  stdin lines "p n border": the index, one a line
//   border     border_at against conv::border_index for every p in -70000 .. 70000 on axes of 1 .. 9
//              under the three borders: {"checked", "failed"}
//   pixels     stdin lines "W H C interp border v0 v1 v2 mode m0 .. m5 hex-bytes-of-the-frame": the warped
//              frame's bytes through resolve and warp_pixel
//   footprint  tile_footprint against every pixel of every tile, on frames up to 40 x 40 under
//              rotations, shrinks, flips and negative scales: {"checked", "failed"}
//   limits     limits_ok and frame_ok, what they accept and the reasons they give: {"checked", "failed"}
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "vf_warp_plan.h"

namespace W = vf::warp;

static double from_bits(uint64_t b) {
  double d;
  std::memcpy(&d, &b, sizeof d);
  return d;
}

static bool read_map(std::istringstream &in, double *m) {
  for (int i = 0; i < 6; ++i) {
    uint64_t b;
    if (!(in >> b)) return false;
    m[i] = from_bits(b);
  }
  return true;
}

static int coords() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    int w, h, interp;
    double m[6];
    if (!(in >> w >> h >> interp) || !read_map(in, m)) return 2;
    const int rd = W::round_delta(interp);
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const W::Coord cx = W::warp_coord(W::row_base(m[1], m[2], y, rd), W::col_delta(m[0], x), interp);
        const W::Coord cy = W::warp_coord(W::row_base(m[4], m[5], y, rd), W::col_delta(m[3], x), interp);
        std::printf("%d %d %d %d ", cx.s, cy.s, cx.f, cy.f);
      }
    std::printf("\n");
  }
  return 0;
}

static int weights() {
  for (int fy = 0; fy < 32; ++fy)
    for (int fx = 0; fx < 32; ++fx) {
      const W::Weights w = W::warp_weights(fx, fy);
      std::printf("%u %u %u %u ", w.w00, w.w01, w.w10, w.w11);
    }
  std::printf("\n");
  return 0;
}

static int border_at_lines() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    int p, n, border;
    if (!(in >> p >> n >> border)) return 2;
    std::printf("%d\n", W::border_at(p, n, border));
  }
  return 0;
}

static int border() {
  long checked = 0, failed = 0;
  for (int n = 1; n <= 9; ++n)
    for (int b = 0; b < 3; ++b)
      for (int p = -70000; p <= 70000; ++p) {
        ++checked;
        if (W::border_at(p, n, b) != vf::conv::border_index(p, n, b)) {
          if (failed++ < 5) std::fprintf(stderr, "border_at(%d, %d, %d) = %d\n", p, n, b, W::border_at(p, n, b));
        }
      }
  std::printf("{\"checked\": %ld, \"failed\": %ld}\n", checked, failed);
  return failed ? 1 : 0;
}

static int pixels() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    int w, h, c, interp, border, v[3], mode;
    double m[6], r[6];
    std::string hex;
    if (!(in >> w >> h >> c >> interp >> border >> v[0] >> v[1] >> v[2] >> mode) || !read_map(in, m) || !(in >> hex)) return 2;
    std::vector<uint8_t> src((size_t)w * h * c);
    if (hex.size() != 2 * src.size()) return 2;
    for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)std::stoi(hex.substr(2 * i, 2), nullptr, 16);
    std::string why;
    if (!W::limits_ok(m, mode, interp, border, v, c, &why) || !W::frame_ok((uint64_t)w, (uint64_t)h, mode, m, &why)) {
      std::fprintf(stderr, "refused: %s\n", why.c_str());
      return 3;
    }
    W::resolve(mode, m, w, h, r);
    const int rd = W::round_delta(interp);
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const W::Coord cx = W::warp_coord(W::row_base(r[1], r[2], y, rd), W::col_delta(r[0], x), interp);
        const W::Coord cy = W::warp_coord(W::row_base(r[4], r[5], y, rd), W::col_delta(r[3], x), interp);
        for (int k = 0; k < c; ++k)
          std::printf("%u ", W::warp_pixel(src.data(), w, h, c, k, cx, cy, interp, border, (uint32_t)v[k]));
      }
    std::printf("\n");
  }
  return 0;
}

// Every first tap of every pixel of the tile, and for linear the second, against the box.
static long footprint_of(const double *m, int interp, int w, int h, int tw, int th, long *failed) {
  long checked = 0;
  const int rd = W::round_delta(interp);
  for (int y0 = 0; y0 < h; y0 += th)
    for (int x0 = 0; x0 < w; x0 += tw) {
      const int x1 = (x0 + tw < w ? x0 + tw : w) - 1, y1 = (y0 + th < h ? y0 + th : h) - 1;
      const W::Box b = W::tile_footprint(m, interp, x0, x1, y0, y1);
      int lo_x = 1 << 30, hi_x = -(1 << 30), lo_y = 1 << 30, hi_y = -(1 << 30);
      for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
          const int sx = W::warp_coord(W::row_base(m[1], m[2], y, rd), W::col_delta(m[0], x), interp).s;
          const int sy = W::warp_coord(W::row_base(m[4], m[5], y, rd), W::col_delta(m[3], x), interp).s;
          const int ex = interp == W::kLinear ? sx + 1 : sx, ey = interp == W::kLinear ? sy + 1 : sy;
          lo_x = sx < lo_x ? sx : lo_x, hi_x = ex > hi_x ? ex : hi_x;
          lo_y = sy < lo_y ? sy : lo_y, hi_y = ey > hi_y ? ey : hi_y;
        }
      ++checked;
      // the box holds every tap, and it is tight: its corners are taps of the tile
      if (b.sx_lo != lo_x || b.sx_hi != hi_x || b.sy_lo != lo_y || b.sy_hi != hi_y) {
        if ((*failed)++ < 5)
          std::fprintf(stderr, "tile (%d..%d, %d..%d) of %d x %d interp %d: box %d..%d x %d..%d, taps %d..%d x %d..%d\n", x0, x1,
                       y0, y1, w, h, interp, b.sx_lo, b.sx_hi, b.sy_lo, b.sy_hi, lo_x, hi_x, lo_y, hi_y);
      }
    }
  return checked;
}

static int footprint() {
  long checked = 0, failed = 0;
  const double pi = 3.14159265358979323846;
  std::vector<std::vector<double>> maps;
  for (int deg = -170; deg <= 180; deg += 35)
    for (double scale : {0.25, 0.5, 0.77, 1.0, 1.3, 3.0}) {
      const double a = scale * std::cos(deg * pi / 180), b = scale * std::sin(deg * pi / 180);
      maps.push_back({a, b, 3.37 - 2 * a, -b, a, 11.2 + b});
    }
  maps.push_back({-1, 0, 39, 0, 1, 0});      // the flips of a 40-wide frame
  maps.push_back({1, 0, 0, 0, -1, 39});
  maps.push_back({-1, 0, 39, 0, -1, 39});
  maps.push_back({-0.5, 0.1, 20.5, 0.2, -1.7, 30.25});   // negative scales with a shear
  maps.push_back({1.25, -0.75, 4, 0.5, -0.3, 9});        // a negative determinant is next
  maps.push_back({0.6, 0.8, -3.5, 0.8, -0.6, 2.5});
  maps.push_back({1, 0, 0.5, 0, 1, 0.5});                // half a pixel
  maps.push_back({1, 0, -1000000, 0, 1, 1000000});       // both coordinates saturate
  maps.push_back({0, 0, 5.5, 0, 0, 7.25});               // a singular map: every pixel reads one place
  const int sizes[][2] = {{40, 40}, {1, 1}, {1, 9}, {9, 1}, {2, 2}, {5, 7}, {37, 23}, {40, 3}};
  const int tiles[][2] = {{8, 8}, {16, 4}, {1, 1}, {5, 3}, {64, 16}, {3, 40}};
  for (const std::vector<double> &m : maps)
    for (int interp = 0; interp < 2; ++interp)
      for (const auto &s : sizes)
        for (const auto &t : tiles) checked += footprint_of(m.data(), interp, s[0], s[1], t[0], t[1], &failed);
  std::printf("{\"checked\": %ld, \"failed\": %ld}\n", checked, failed);
  return failed ? 1 : 0;
}

static int limits() {
  long checked = 0, failed = 0;
  auto expect = [&](bool got, bool want, const std::string &why, const char *word, const char *what) {
    ++checked;
    if (got != want || (!want && why.find(word) == std::string::npos)) {
      ++failed;
      std::fprintf(stderr, "%s: got %d want %d, reason \"%s\" lacks \"%s\"\n", what, (int)got, (int)want, why.c_str(), word);
    }
  };
  const double id[6] = {1, 0, 0, 0, 1, 0};
  const int zero[3] = {0, 0, 0}, colour[3] = {1, 128, 255};
  std::string why;
  for (int c : {1, 3})
    for (int mode = 0; mode < 4; ++mode)
      for (int interp = 0; interp < 2; ++interp)
        for (int b = 0; b < 3; ++b) {
          why.clear();
          expect(W::limits_ok(id, mode, interp, b, colour, c, &why), true, why, "", "accepted");
        }
  expect(W::limits_ok(nullptr, W::kFlipH, 0, 0, zero, 3, &why), true, why, "", "a flip reads no m");
  expect(W::limits_ok(id, 0, 0, 0, zero, 2, &why), false, why, "channels=2", "channels 2");
  expect(W::limits_ok(id, 0, 0, 0, zero, 4, &why), false, why, "channels=4", "channels 4");
  expect(W::limits_ok(id, 4, 0, 0, zero, 3, &why), false, why, "mode=4", "mode 4");
  expect(W::limits_ok(id, -1, 0, 0, zero, 3, &why), false, why, "mode=-1", "mode -1");
  expect(W::limits_ok(id, 0, 2, 0, zero, 3, &why), false, why, "interp=2", "interp 2");
  expect(W::limits_ok(id, 0, -1, 0, zero, 3, &why), false, why, "interp=-1", "interp -1");
  expect(W::limits_ok(id, 0, 0, 3, zero, 3, &why), false, why, "unknown border 3", "border 3");
  expect(W::limits_ok(id, 0, 0, -1, zero, 3, &why), false, why, "unknown border -1", "border -1");
  expect(W::limits_ok(id, 0, 0, 0, nullptr, 3, &why), false, why, "value is NULL", "no value");
  expect(W::limits_ok(nullptr, 0, 0, 0, zero, 3, &why), false, why, "m is NULL", "no m");
  for (int k = 0; k < 3; ++k) {
    int v[3] = {0, 0, 0};
    v[k] = 256;
    expect(W::limits_ok(id, 0, 0, 0, v, 3, &why), false, why, ("value[" + std::to_string(k) + "]=256").c_str(), "value 256");
    v[k] = -1;
    expect(W::limits_ok(id, 0, 0, 0, v, 3, &why), false, why, ("value[" + std::to_string(k) + "]=-1").c_str(), "value -1");
  }
  for (int k = 0; k < 6; ++k)
    for (double bad : {std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(),
                       std::numeric_limits<double>::quiet_NaN()}) {
      double m[6] = {1, 0, 0, 0, 1, 0};
      m[k] = bad;
      expect(W::limits_ok(m, 0, 0, 0, zero, 3, &why), false, why, ("m[" + std::to_string(k) + "] is not finite").c_str(), "finite");
    }
  // frames
  expect(W::frame_ok(32767, 32767, 0, id, &why), true, why, "", "the largest frame");
  expect(W::frame_ok(32768, 10, 0, id, &why), false, why, "a side is at most 32767", "width 32768");
  expect(W::frame_ok(10, 32768, 0, id, &why), false, why, "a side is at most 32767", "height 32768");
  expect(W::frame_ok(32767, 32767, W::kFlipBoth, nullptr, &why), true, why, "", "the largest flip");
  expect(W::frame_ok(1, 1, 0, id, &why), true, why, "", "one pixel");
  {  // |m0| (W - 1) 1024 < 2^30: 16384 * 64 * 1024 is 2^30 exactly
    double m[6] = {16384.0, 0, 0, 0, 1, 0};
    expect(W::frame_ok(65, 10, 0, m, &why), false, why, "m[0]", "m0 at the limit");
    m[0] = -m[0];
    expect(W::frame_ok(65, 10, 0, m, &why), false, why, "m[0]", "-m0 at the limit");
    expect(W::frame_ok(64, 10, 0, m, &why), true, why, "", "m0 below the limit on a narrower frame");
    double n[6] = {1, 0, 0, 16384.0, 1, 0};
    expect(W::frame_ok(65, 10, 0, n, &why), false, why, "m[3]", "m3 at the limit");
    expect(W::frame_ok(1, 10, 0, n, &why), true, why, "", "m3 on one column");
  }
  {  // |m1 y + m2| 1024 + 512 < 2^30
    double m[6] = {1, 0, 1048575.5, 0, 1, 0};
    expect(W::frame_ok(10, 10, 0, m, &why), false, why, "m[2]", "m2 at the limit");
    m[2] = 1048575.0;
    expect(W::frame_ok(10, 10, 0, m, &why), true, why, "", "m2 below the limit");
    m[2] = -1048575.5;
    expect(W::frame_ok(10, 10, 0, m, &why), false, why, "m[2]", "-m2 at the limit");
    double n[6] = {1, 0, 0, 0, 1, 1048575.5};
    expect(W::frame_ok(10, 10, 0, n, &why), false, why, "m[5]", "m5 at the limit");
    double r[6] = {1, 200000, 0, 0, 1, 0};  // the last row leaves the range, the first does not
    expect(W::frame_ok(10, 7, 0, r, &why), false, why, "at row 6", "m1 at the last row");
    expect(W::frame_ok(10, 5, 0, r, &why), true, why, "", "m1 on fewer rows");
    double q[6] = {1, 0, 0, 0, -200000, 0};
    expect(W::frame_ok(10, 7, 0, q, &why), false, why, "m[4]", "m4 at the last row");
    double t[6] = {1, 0, 1000000, 0, 1, -1000000};  // the saturating translation is inside the limits
    expect(W::frame_ok(5, 5, 0, t, &why), true, why, "", "a translation of a million");
  }
  // resolve
  double r[6];
  W::resolve(W::kFlipH, nullptr, 7, 5, r);
  ++checked, failed += !(r[0] == -1 && r[1] == 0 && r[2] == 6 && r[3] == 0 && r[4] == 1 && r[5] == 0);
  W::resolve(W::kFlipV, nullptr, 7, 5, r);
  ++checked, failed += !(r[0] == 1 && r[1] == 0 && r[2] == 0 && r[3] == 0 && r[4] == -1 && r[5] == 4);
  W::resolve(W::kFlipBoth, nullptr, 7, 5, r);
  ++checked, failed += !(r[0] == -1 && r[1] == 0 && r[2] == 6 && r[3] == 0 && r[4] == -1 && r[5] == 4);
  // the conversion saturates and never overflows
  ++checked, failed += W::round_to_int(1e300) != 2147483647;
  ++checked, failed += W::round_to_int(-1e300) != -2147483647 - 1;
  ++checked, failed += W::round_to_int(0.5) != 0 || W::round_to_int(1.5) != 2 || W::round_to_int(-0.5) != 0 || W::round_to_int(2.5) != 2;
  ++checked, failed += W::round_to_int(std::numeric_limits<double>::quiet_NaN()) != 0;
  std::printf("{\"checked\": %ld, \"failed\": %ld}\n", checked, failed);
  return failed ? 1 : 0;
}

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "coords") return coords();
  if (mode == "weights") return weights();
  if (mode == "border_at") return border_at_lines();
  if (mode == "border") return border();
  if (mode == "pixels") return pixels();
  if (mode == "footprint") return footprint();
  if (mode == "limits") return limits();
  std::fprintf(stderr, "usage: warp_plan_check coords|weights|border_at|border|pixels|footprint|limits\n");
  return 2;
}
