// sep_plan_check — csrc/vf_sep_plan.h on the CPU.  Modes:
//   limits     what limits_ok accepts and refuses, with the reason
//   divide     the division by a constant, for every odd d <= 1023 over the whole clamped range
//              and beyond it on both sides, and the reciprocal that splits a staging item
//   geometry   for every (kw, kh), channel count, sum width and tile height the launcher can
//              pick: the halo holds the taps' reach, the LDS is what the parts add up to and
//              never exceeds kMaxLds, and the results fit under the staged bytes
// Each prints one JSON line; exit status 1 when a check failed.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "vf_sep_plan.h"

using namespace vf::sep;

namespace {

long g_failed = 0, g_checked = 0;
#define CHECK(c)                                           \
  do {                                                     \
    ++g_checked;                                           \
    if (!(c)) {                                            \
      if (++g_failed < 20) std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
    }                                                      \
  } while (0)

bool refused(const int16_t *kx, int kw, const int16_t *ky, int kh, int shift, int d, int rounding, int border,
             const char *reason) {
  std::string why;
  return !limits_ok(kx, kw, ky, kh, shift, d, rounding, border, &why) && why.find(reason) != std::string::npos;
}

int run_limits() {
  std::vector<int16_t> ones(33, 1), big(3, 86), edge(31, 0);
  const int16_t *o = ones.data();
  std::string why;
  for (int n = 1; n <= 31; n += 2) CHECK(limits_ok(o, n, o, 32 - n, 0, 1, 0, 0, &why));
  CHECK(limits_ok(o, 31, o, 31, 0, 961, 0, 0, &why) && limits_ok(o, 3, o, 3, 16, 1, 1, 2, &why));
  CHECK(limits_ok(o, 1, o, 1, 0, 1023, 0, 1, &why));
  CHECK(refused(nullptr, 3, o, 3, 0, 1, 0, 0, "NULL") && refused(o, 3, nullptr, 3, 0, 1, 0, 0, "NULL"));
  for (int bad : {0, 2, 30, 32, 33, -3}) {
    CHECK(refused(o, bad, o, 3, 0, 1, 0, 0, "odd and at most 31"));
    CHECK(refused(o, 3, o, bad, 0, 1, 0, 0, "odd and at most 31"));
  }
  edge[0] = 256, edge[30] = -256;  // 512 * 128 = 65536: allowed; one more is not
  std::vector<int16_t> k128(31, 0), k129(31, 0);
  k128[3] = 128, k129[3] = -129;
  CHECK(limits_ok(edge.data(), 31, k128.data(), 31, 0, 1, 0, 0, &why));
  CHECK(refused(edge.data(), 31, k129.data(), 31, 0, 1, 0, 0, "exceeds 65536"));
  CHECK(refused(big.data(), 3, big.data(), 3, 0, 1, 0, 0, "66564 exceeds 65536"));
  CHECK(refused(o, 3, o, 3, 17, 1, 0, 0, "shift=17") && refused(o, 3, o, 3, -1, 1, 0, 0, "shift=-1"));
  for (int d : {0, -1, 2, 4, 1024, 1025, 960}) CHECK(refused(o, 3, o, 3, 0, d, 0, 0, "divisor="));
  CHECK(refused(o, 3, o, 3, 1, 9, 0, 0, "together"));
  CHECK(refused(o, 3, o, 3, 0, 9, 2, 0, "unknown rounding 2") && refused(o, 3, o, 3, 0, 9, -1, 0, "unknown rounding"));
  CHECK(refused(o, 3, o, 3, 0, 9, 0, 3, "unknown border 3") && refused(o, 3, o, 3, 0, 9, 0, -1, "unknown border"));
  // the 16-bit sums: 255 * sum|ky| < 2^15
  CHECK(narrow_fits(k128.data(), 31) && !narrow_fits(k129.data(), 31) && narrow_fits(o, 31));
  std::printf("{\"checked\": %ld, \"failed\": %ld}\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}

int run_divide() {
  long values = 0;
  int divisors = 0;
  for (int d = 1; d <= kMaxDivisor; d += 2) {
    const Divide v = divide_by(d);
    ++divisors;
    CHECK(v.top == 255 * d + (d - 1) / 2 && 2L * v.top + d < (1L << 20));
    for (int acc = -2 * d; acc <= v.top + 2 * d; ++acc) {  // the clamped range, and past it on both sides
      const long n = 2L * acc + d;
      long q = n >= 0 ? n / (2L * d) : -((-n + 2L * d - 1) / (2L * d));  // floor
      q = q < 0 ? 0 : q > 255 ? 255 : q;
      ++values;
      if (divide(v, acc) != (int)q) CHECK(divide(v, acc) == (int)q);
    }
    for (int acc : {-(1 << 24), (1 << 24), -1, 0}) CHECK(divide(v, acc) == (acc > 0 ? 255 : 0));
  }
  g_checked += values;
  // the split of a staging item by the pieces of a row, as the kernel does it
  for (uint32_t n = 16; n <= 22; ++n)
    for (uint32_t x = 0; x < 62 * 22 + 256; ++x) CHECK(div_recip(x, recip(n)) == x / n);
  std::printf("{\"divisors\": %d, \"values\": %ld, \"checked\": %ld, \"failed\": %ld}\n", divisors, values, g_checked,
              g_failed);
  return g_failed ? 1 : 0;
}

int run_geometry() {
  int cases = 0, max_lds = 0;
  for (int kw = 1; kw <= kMaxSide; kw += 2)
    for (int kh = 1; kh <= kMaxSide; kh += 2)
      for (int c : {1, 3})
        for (int narrow = 0; narrow < 2; ++narrow)
          for (int rows : {tile_rows(kh), 16, 24, 32}) {
            // the launcher takes another height than the plan's only where the widest case fits
            if (rows != tile_rows(kh) && geometry(kMaxSide, kh, 3, false, rows).lds_bytes > kMaxLds) continue;
            const Geometry g = geometry(kw, kh, c, narrow, rows);
            ++cases;
            CHECK(rows_ok(g.rows));
            CHECK(g.halo % 16 == 0 && g.halo >= (kw / 2) * c && g.halo <= 48);
            CHECK(g.stage_bytes == kTileBytes + 2 * g.halo && g.stage_bytes % 16 == 0 && g.stage_bytes / 16 <= 22);
            CHECK(g.stage_rows == g.rows + 2 * (kh / 2) && g.stage_rows <= 62);
            CHECK(g.elem_bytes == (narrow ? 2 : 4));
            CHECK(g.lds_bytes == g.stage_rows * g.stage_bytes + g.rows * g.stage_bytes * g.elem_bytes);
            CHECK(g.lds_bytes <= kMaxLds);
            CHECK(g.rows * kTileBytes <= g.stage_rows * g.stage_bytes);  // the results go over the staged bytes
            CHECK((g.stage_rows * g.stage_bytes) % 16 == 0);             // the sums start 16-B aligned
            // the last tap of the last byte of a row of sums stays inside that row
            CHECK(g.halo + kTileBytes - 1 + (kw / 2) * c < g.stage_bytes && g.halo - (kw / 2) * c >= 0);
            if (g.lds_bytes > max_lds) max_lds = g.lds_bytes;
          }
  CHECK(tile_rows(1) == 16 && tile_rows(7) == 16 && tile_rows(9) == 16 && tile_rows(31) == 16);
  std::printf("{\"cases\": %d, \"max_lds\": %d, \"checked\": %ld, \"failed\": %ld}\n", cases, max_lds, g_checked, g_failed);
  return g_failed ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
  const char *mode = argc > 1 ? argv[1] : "";
  if (!std::strcmp(mode, "limits")) return run_limits();
  if (!std::strcmp(mode, "divide")) return run_divide();
  if (!std::strcmp(mode, "geometry")) return run_geometry();
  std::fprintf(stderr, "usage: sep_plan_check limits | divide | geometry\n");
  return 2;
}
