// conv_bands_check.cc — CPU checks of csrc/vf_conv_border.h and csrc/vf_conv_bands.h (built by
// tests/test_conv_bands.py with -fsanitize=address,undefined).
//
//   conv_bands_check border
//       border_index against its definition for n in {1, 2, 3, 8}, p in [-8, n + 8), every border.
//   conv_bands_check grid
//       the bands check below over a grid of small frames, radii and capacities.
//   conv_bands_check bands W H C ry capacity
//       the bands of one frame: they tile [0, H) once and in order, each fits the capacity and
//       uploads [max(0, y0 - ry), min(H, y1 + ry)), and a reference stencil run band by band --
//       reading only the band's uploaded rows, the border resolved in frame coordinates -- equals
//       the whole-frame result for all three borders.  A capacity that cannot hold one output row
//       with its halo must be reported as an error (and in finite time).
// Prints one JSON object; exit status 0 when nothing failed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vf_conv_bands.h"
#include "vf_conv_border.h"

using vf::conv::Band;
using vf::conv::border_index;

static int g_failed = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++g_failed;                   \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
    }                               \
  } while (0)

// the definition, written out independently
static int border_def(int p, int n, int border) {
  if (p >= 0 && p < n) return p;
  if (border == vf::conv::kConstant) return -1;
  if (border == vf::conv::kReplicate) return p < 0 ? 0 : n - 1;
  if (n == 1) return 0;
  const int period = 2 * n - 2;  // reflect-101 is periodic: ... 2 1 | 0 1 .. n-1 | n-2 .. 1 0 | 1 ...
  int q = ((p % period) + period) % period;
  return q < n ? q : period - q;
}

static int check_border() {
  const int ns[] = {1, 2, 3, 8};
  int checked = 0;
  for (int n : ns)
    for (int b = 0; b < 3; ++b)
      for (int p = -8; p < n + 8; ++p, ++checked)
        CHECK(border_index(p, n, b) == border_def(p, n, b), "border_index(%d, %d, %d) = %d, want %d", p, n, b,
              border_index(p, n, b), border_def(p, n, b));
  printf("{\"checked\": %d, \"failed\": %d}\n", checked, g_failed);
  return g_failed ? 1 : 0;
}

// a 3 x (2 ry + 1) stencil with distinct weights; `rows` holds frame rows [s0, s1) only
static int stencil(const std::vector<uint8_t> &rows, int s0, int s1, int W, int H, int C, int ry, int border, int y,
                   int xb) {
  int acc = 0;
  const int x = xb / C, c = xb % C;
  for (int j = -ry; j <= ry; ++j) {
    const int fy = border_index(y + j, H, border);
    if (fy < 0) continue;
    if (fy < s0 || fy >= s1) {
      CHECK(false, "row %d of output row %d is outside the uploaded rows [%d, %d)", fy, y, s0, s1);
      continue;
    }
    for (int i = -1; i <= 1; ++i) {
      const int fx = border_index(x + i, W, border);
      if (fx < 0) continue;
      acc += (3 * (j + ry) + (i + 1) + 1) * rows[((size_t)(fy - s0) * W + fx) * C + c];
    }
  }
  return acc;
}

// *error: bands() refused the frame; *nb: how many bands it gave
static void check_bands(int W, int H, int C, int ry, size_t cap, bool *error, size_t *nb) {
  *error = false;
  *nb = 0;
  std::vector<Band> bs;
  const bool ok = vf::conv::bands(W, H, C, ry, cap, &bs);
  const size_t row = (size_t)W * C;
  // does every output row with its halo fit?  (the rows a band of one row uploads)
  bool fits = W > 0 && H > 0 && C > 0;
  for (int y = 0; fits && y < H; ++y) {
    const int s0 = y - ry > 0 ? y - ry : 0, s1 = y + 1 + ry < H ? y + 1 + ry : H;
    if ((size_t)(s1 - s0) * row > cap) fits = false;
  }
  if (!ok) {
    CHECK(bs.empty(), "an error with %zu bands", bs.size());
    CHECK(!fits, "error although every row with its halo fits (%d %d %d %d %zu)", W, H, C, ry, cap);
    *error = true;
    return;
  }
  CHECK(fits, "bands although a row with its halo does not fit");
  int y = 0;
  for (const Band &b : bs) {
    CHECK(b.y0 == y && b.y1 > b.y0 && b.y1 <= H, "band [%d, %d) after row %d", b.y0, b.y1, y);
    const int s0 = b.y0 - ry > 0 ? b.y0 - ry : 0, s1 = b.y1 + ry < H ? b.y1 + ry : H;
    CHECK(b.s0 == s0 && b.s1 == s1, "band [%d, %d) uploads [%d, %d), want [%d, %d)", b.y0, b.y1, b.s0, b.s1, s0, s1);
    CHECK((size_t)(b.s1 - b.s0) * row <= cap, "band [%d, %d) uploads %zu bytes > %zu", b.y0, b.y1,
          (size_t)(b.s1 - b.s0) * row, cap);
    y = b.y1;
    if (g_failed) break;
  }
  CHECK(y == H, "bands end at row %d of %d", y, H);
  if (!g_failed) {
    std::vector<uint8_t> frame((size_t)H * row);
    uint32_t s = 12345u + (uint32_t)(W * 31 + H * 7 + C);
    for (uint8_t &v : frame) v = (uint8_t)((s = s * 1664525u + 1013904223u) >> 24);
    for (int border = 0; border < 3 && !g_failed; ++border)
      for (const Band &b : bs) {
        // the band's own copy of its uploaded rows: a read outside it is a sanitizer error
        const std::vector<uint8_t> rows(frame.begin() + (size_t)b.s0 * row, frame.begin() + (size_t)b.s1 * row);
        for (int yy = b.y0; yy < b.y1; ++yy)
          for (int xb = 0; xb < (int)row; ++xb) {
            const int got = stencil(rows, b.s0, b.s1, W, H, C, ry, border, yy, xb);
            const int want = stencil(frame, 0, H, W, H, C, ry, border, yy, xb);
            CHECK(got == want, "border %d band [%d, %d) row %d byte %d: %d, want %d", border, b.y0, b.y1, yy, xb, got,
                  want);
            if (g_failed) break;
          }
      }
  }
  *nb = bs.size();
}

// every (W, H, C, ry) of a small grid at capacities of 0 .. H + 1 whole rows, one byte less and more
static int check_grid() {
  const int Ws[] = {1, 2, 5}, Hs[] = {1, 2, 3, 4, 7, 8, 9, 20}, Cs[] = {1, 3};
  long cases = 0, errors = 0, banded = 0;
  for (int W : Ws)
    for (int H : Hs)
      for (int C : Cs)
        for (int ry = 0; ry <= 3 && !g_failed; ++ry) {
          const size_t row = (size_t)W * C;
          for (int k = 0; k <= H + 1; ++k)
            for (int d = -1; d <= 1; ++d) {
              if (k == 0 && d < 0) continue;
              bool err = false;
              size_t nb = 0;
              check_bands(W, H, C, ry, row * k + d, &err, &nb);
              ++cases;
              errors += err;
              banded += nb > 1;
            }
        }
  printf("{\"cases\": %ld, \"errors\": %ld, \"multi_band\": %ld, \"failed\": %d}\n", cases, errors, banded, g_failed);
  return g_failed ? 1 : 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "border") == 0) return check_border();
  if (argc == 2 && strcmp(argv[1], "grid") == 0) return check_grid();
  if (argc == 7 && strcmp(argv[1], "bands") == 0) {
    bool err = false;
    size_t nb = 0;
    check_bands(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), (size_t)strtoull(argv[6], nullptr, 10), &err, &nb);
    printf("{\"error\": %s, \"bands\": %zu, \"failed\": %d}\n", err ? "true" : "false", nb, g_failed);
    return g_failed ? 1 : 0;
  }
  fprintf(stderr, "usage: conv_bands_check border | grid | bands W H C ry capacity\n");
  return 2;
}
