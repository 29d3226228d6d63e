// tile_plan_check.cc — csrc/vf_tile_plan.h on the CPU (built by tests/test_tile_plan.py with
// -fsanitize=address,undefined).
//
//   tile_plan_check rows NROWS   the row chunks of NROWS output rows cover [0, NROWS) once and in
//                                order, each of 1 .. 65535 * 16 rows; prints {"chunks", "failed"}
//   tile_plan_check square       for every odd (kw, kh) up to 7: the square is the smallest of 3, 5,
//                                7 that holds the kernel, and square_at puts each weight where the
//                                launchers' loops did and where centring says: the kernel's centre
//                                on the square's, every entry as far from it as in the kernel;
//                                prints {"kernels", "failed"}
//   tile_plan_check checks       sides_ok, border_ok and rows_ok against their definitions; prints
//                                {"checked", "failed"}
// Exit status 1 when a check failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vf_tile_plan.h"

static int g_failed = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (++g_failed <= 20) {                     \
        std::fprintf(stderr, "FAILED %s: ", #cond); \
        std::fprintf(stderr, __VA_ARGS__);        \
        std::fprintf(stderr, "\n");               \
      }                                           \
    }                                             \
  } while (0)

using namespace vf::tile;

static int rows(int nrows) {
  static_assert(kMaxRows == 65535 * 16, "the grid's y limit times the tile's rows");
  const std::vector<RowChunk> cs = row_chunks(nrows);
  std::vector<uint8_t> seen((size_t)(nrows > 0 ? nrows : 0), 0);  // exactly nrows: a row past them is ASan's
  int at = 0;
  for (size_t k = 0; k < cs.size(); ++k) {
    CHECK(cs[k].done == at, "chunk %zu starts at %d, not %d", k, cs[k].done, at);
    CHECK(cs[k].m >= 1 && cs[k].m <= kMaxRows, "chunk %zu: %d rows", k, cs[k].m);
    CHECK(cs[k].m <= nrows - at, "chunk %zu: %d rows with %d left", k, cs[k].m, nrows - at);
    if (cs[k].done != at || cs[k].m < 1 || cs[k].m > nrows - at) break;
    if (k + 1 < cs.size()) CHECK(cs[k].m == kMaxRows, "chunk %zu: short (%d) before the end", k, cs[k].m);
    for (int y = at; y < at + cs[k].m; ++y) ++seen[(size_t)y];
    at += cs[k].m;
  }
  CHECK(at == (nrows > 0 ? nrows : 0), "chunks end at row %d of %d", at, nrows);
  size_t bad = 0;
  for (uint8_t s : seen) bad += s != 1;
  CHECK(bad == 0, "%zu rows not covered exactly once", bad);
  std::printf("{\"chunks\": %zu, \"failed\": %d}\n", cs.size(), g_failed);
  return g_failed ? 1 : 0;
}

static int square() {
  int kernels = 0;
  for (int kh = 1; kh <= 7; kh += 2)
    for (int kw = 1; kw <= 7; kw += 2) {
      ++kernels;
      const int ks = square_side(kw, kh), big = kw > kh ? kw : kh;
      CHECK(ks == (big <= 3 ? 3 : big <= 5 ? 5 : 7), "%d x %d: side %d", kw, kh, ks);
      if (ks < big || ks > 7) continue;
      // the launchers' loops before the header: offsets (ox, oy), then row-major in the square
      std::vector<int> was((size_t)(ks * ks), -1), now((size_t)(ks * ks), -1);
      const int ox = (ks - kw) / 2, oy = (ks - kh) / 2;
      for (int j = 0; j < kh; ++j)
        for (int i = 0; i < kw; ++i) was[(size_t)((j + oy) * ks + i + ox)] = j * kw + i;
      for (int j = 0; j < kh; ++j)
        for (int i = 0; i < kw; ++i) {
          const int at = square_at(ks, kw, kh, j, i);
          CHECK(at >= 0 && at < ks * ks, "%d x %d entry (%d, %d): position %d", kw, kh, j, i, at);
          if (at < 0 || at >= ks * ks) continue;
          CHECK(now[(size_t)at] == -1, "%d x %d entry (%d, %d): position %d taken twice", kw, kh, j, i, at);
          now[(size_t)at] = j * kw + i;
          // tap (j, i) is (j - kh / 2, i - kw / 2) from the anchor, which sits at the square's centre
          CHECK(at == (ks / 2 + j - kh / 2) * ks + ks / 2 + i - kw / 2, "%d x %d entry (%d, %d): not centred", kw, kh, j, i);
        }
      CHECK(was == now, "%d x %d: the weights moved", kw, kh);
    }
  std::printf("{\"kernels\": %d, \"failed\": %d}\n", kernels, g_failed);
  return g_failed ? 1 : 0;
}

static int checks() {
  int n = 0;
  for (int kw = -1; kw <= 9; ++kw)
    for (int kh = -1; kh <= 9; ++kh, ++n) {
      const bool want = kw >= 1 && kw <= 7 && kw % 2 == 1 && kh >= 1 && kh <= 7 && kh % 2 == 1;
      CHECK(sides_ok(kw, kh) == want, "sides_ok(%d, %d)", kw, kh);
    }
  for (int b = -2; b <= 4; ++b, ++n) CHECK(border_ok(b) == (b >= 0 && b <= 2), "border_ok(%d)", b);
  int x = 0;
  const void *p = &x;
  struct {
    const void *src, *dst;
    int w, c, h, y0, nrows, s0, nsrc;
    bool ok;
  } const cases[] = {
      {p, p, 640, 3, 480, 0, 480, 0, 480, true},     {p, p, 640, 1, 480, 470, 10, 467, 13, true},
      {nullptr, p, 640, 3, 480, 0, 480, 0, 480, false}, {p, nullptr, 640, 3, 480, 0, 480, 0, 480, false},
      {p, p, 640, 2, 480, 0, 480, 0, 480, false},    {p, p, 640, 4, 480, 0, 480, 0, 480, false},
      {p, p, 0, 3, 480, 0, 480, 0, 480, false},      {p, p, 640, 3, 0, 0, 0, 0, 0, false},
      {p, p, 640, 3, 480, -1, 10, 0, 480, false},    {p, p, 640, 3, 480, 471, 10, 0, 480, false},
      {p, p, 640, 3, 480, 0, 0, 0, 480, false},      {p, p, 640, 3, 480, 0, 480, -1, 480, false},
      {p, p, 640, 3, 480, 0, 480, 1, 480, false},    {p, p, 640, 3, 480, 0, 480, 0, 0, false},
      {p, p, 640, 3, 0x7FFFFFFF, 1, 0x7FFFFFFF, 0, 1, false},  // y0 + nrows overflows an int
      {p, p, 0x7FFFFFFF, 1, 1, 0, 1, 0, 1, true},    {p, p, 0x2AAAAAAA, 3, 1, 0, 1, 0, 1, true},
      {p, p, 0x2AAAAAAB, 3, 1, 0, 1, 0, 1, false},   // W * C = 2^31 + 1
  };
  for (const auto &c : cases) {
    ++n;
    CHECK(rows_ok(c.src, c.dst, c.w, c.c, c.h, c.y0, c.nrows, c.s0, c.nsrc) == c.ok, "rows_ok case %d", n);
  }
  std::printf("{\"checked\": %d, \"failed\": %d}\n", n, g_failed);
  return g_failed ? 1 : 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !std::strcmp(argv[1], "rows")) return rows(std::atoi(argv[2]));
  if (argc == 2 && !std::strcmp(argv[1], "square")) return square();
  if (argc == 2 && !std::strcmp(argv[1], "checks")) return checks();
  std::fprintf(stderr, "usage: %s rows NROWS | square | checks\n", argv[0]);
  return 2;
}
