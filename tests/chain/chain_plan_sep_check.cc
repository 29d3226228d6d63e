// chain_plan_sep_check — csrc/vf_chain_plan.h's separable step (kind 7) on the CPU.  Modes:
//   validate   kind 7 is accepted on 1 and 3 channels with tap counts up to 31, bad sides are
//              refused with a message of their own; kinds 4, 6, 9 and -1 stay "unknown kind N";
//              the conv and rank limit and message do not change
//   plan       never in place, no fold across a separable step, single_kind, radius kh / 2, reach
//   grid       a scalar model of the steps, band by band on only the rows the plan says exist,
//              equals the whole frame for programs with separable steps
// Each prints one JSON line; exit status 1 when a check failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vf_chain_plan.h"
#include "vf_conv_bands.h"
#include "vf_conv_border.h"

using namespace vf::chain;

namespace {

int g_failed = 0, g_checked = 0;
#define CHECK(c)                                           \
  do {                                                     \
    ++g_checked;                                           \
    if (!(c)) {                                            \
      ++g_failed;                                          \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
    }                                                      \
  } while (0)

enum { kErode = 0, kDilate = 1, kMedian = 2 };  // VF_RANK_*

Step table1(int a, int seed) {
  Step s;
  s.kind = kTable, s.a = a, s.channels = 1;
  s.table.resize(256);
  for (int v = 0; v < 256; ++v) s.table[v] = (uint8_t)(seed == 0 ? 255 - v : (v * 7 + seed) & 255);
  return s;
}
Step rank(int a, int op, int k, int border) {
  Step s;
  s.kind = kRank, s.a = a, s.op = op, s.kw = k, s.kh = k, s.border = border;
  s.element.assign((size_t)k * k, 1);
  return s;
}
Step bin(int op, int a, int b) {
  Step s;
  s.kind = kBinary, s.op = op, s.a = a, s.b = b;
  return s;
}
// kw x kh signed taps; divisor > 1: a mean-like scale, else a shift with the rounding
Step sep(int a, int kw, int kh, int border, int shift, int divisor = 1, int rounding = kRoundHalfEven) {
  Step s;
  s.kind = kSep, s.a = a, s.op = rounding, s.kw = kw, s.kh = kh, s.border = border, s.shift = shift, s.divisor = divisor;
  for (int i = 0; i < kw; ++i) s.taps_x.push_back((int16_t)(divisor > 1 ? 1 : (i * 5) % 7 - 2));
  for (int j = 0; j < kh; ++j) s.taps_y.push_back((int16_t)(divisor > 1 ? 1 : (j * 3) % 5 - 1));
  return s;
}

bool refused(const Program &p, int channels, const char *reason) {
  std::string why;
  return !validate(p, channels, &why) && why.find(reason) != std::string::npos;
}

int run_validate() {
  const int B = vf::conv::kReflect101;
  Program p;
  std::string why;
  CHECK(kSep == 7 && kMix == 5 && kTable == 0 && kConv == 1 && kRank == 2 && kBinary == 3 && kMaxSepSide == 31 && kMaxSide == 7);
  for (int ch : {1, 3})
    for (int kw : {1, 3, 9, 31})
      for (int kh : {1, 5, 31}) {
        p.steps = {sep(0, kw, kh, B, 3)};
        CHECK(validate(p, ch, &why));
      }
  p.steps = {sep(0, 31, 31, B, 0, 961)};
  CHECK(validate(p, 3, &why));
  const char *own = "a separable step's tap counts are odd and at most 31";
  for (int bad : {0, 2, 32, 33, -1}) {
    p.steps = {sep(0, 3, 3, B, 0)};
    p.steps[0].kw = bad;
    CHECK(refused(p, 3, own));
    p.steps = {sep(0, 3, 3, B, 0)};
    p.steps[0].kh = bad;
    CHECK(refused(p, 1, own));
  }
  p.steps = {sep(0, 3, 5, B, 0)};
  p.steps[0].taps_x.pop_back();
  CHECK(refused(p, 3, "the taps do not hold kw and kh entries"));
  p.steps = {sep(0, 3, 5, B, 0)};
  p.steps[0].taps_y.push_back(1);
  CHECK(refused(p, 3, "the taps do not hold kw and kh entries"));
  p.steps = {sep(0, 3, 3, B, 2)};
  p.steps[0].op = 2;
  CHECK(refused(p, 3, "unknown rounding 2"));
  // the conv and rank limit and its words are what they were
  p.steps = {rank(0, kErode, 9, B)};
  CHECK(refused(p, 3, "step 1: sides are odd and at most 7"));
  p.steps = {rank(0, kErode, 7, B)};
  CHECK(validate(p, 3, &why));
  for (int k : {4, 6, 9, -1}) {  // not kinds
    p.steps = {sep(0, 3, 3, B, 0)};
    p.steps[0].kind = k;
    CHECK(refused(p, 3, ("step 1: unknown kind " + std::to_string(k)).c_str()));
    CHECK(refused(p, 1, ("step 1: unknown kind " + std::to_string(k)).c_str()));
  }
  p.steps = {sep(1, 3, 3, B, 0)};  // operands as for every step
  CHECK(refused(p, 3, "operand a = 1 is not an earlier value"));
  p.steps = {sep(0, 3, 3, B, 0), sep(0, 3, 3, B, 0)};
  CHECK(refused(p, 3, "value 1 is read by no step"));
  std::printf("{\"checked\": %d, \"failed\": %d}\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}

int run_plan() {
  const int B = vf::conv::kReplicate;
  Program p;
  // never in place, even over an operand that dies at the step
  p.steps = {sep(0, 5, 31, B, 4)};
  Buffers b = assign_buffers(p);
  CHECK(b.of[1] != b.of[0] && b.count == 2);
  CHECK(is_neighbourhood(p.steps[0]) && radius(p.steps[0]) == 15 && reach(p) == 15);
  CHECK(single_kind(p) == kSep && single_kind(fold(p)) == kSep);
  p.steps = {sep(0, 31, 1, B, 4)};  // 31 taps across, 1 down: no vertical reach
  CHECK(radius(p.steps[0]) == 0 && reach(p) == 0 && assign_buffers(p).of[1] != 0);
  p.steps = {table1(0, 3), sep(1, 3, 3, B, 2), table1(2, 0)};
  b = assign_buffers(p);
  CHECK(b.of[1] == b.of[0] && b.of[2] != b.of[1] && b.of[3] == b.of[2]);  // the tables in place, the sep not
  // no fold across a separable step, and none of two of them
  Program f = fold(p);
  CHECK(f.size() == 3 && f.steps[0].kind == kTable && f.steps[1].kind == kSep && f.steps[2].kind == kTable);
  CHECK(f.steps[1].a == 1 && f.steps[2].a == 2 && f.steps[1].taps_x == p.steps[1].taps_x && f.steps[1].taps_y == p.steps[1].taps_y);
  p.steps = {sep(0, 3, 3, B, 2), sep(1, 3, 5, B, 0, 15)};
  f = fold(p);
  CHECK(f.size() == 2 && f.steps[1].divisor == 15 && f.steps[0].divisor == 1);
  CHECK(single_kind(p) == -1);
  p.steps = {table1(0, 0), table1(1, 5), sep(2, 3, 3, B, 1), table1(3, 7), table1(4, 0)};  // the tables on each side fold
  f = fold(p);
  CHECK(f.size() == 3 && f.steps[1].kind == kSep && f.steps[1].a == 1 && f.steps[2].a == 2);
  // a chain's reach passes 100 rows: seven steps of 31 vertical taps
  p.steps.clear();
  for (int i = 0; i < 7; ++i) p.steps.push_back(sep(i, 1, 31, B, 3));
  std::string why;
  CHECK(validate(p, 3, &why) && reach(p) == 105);
  const std::vector<Rows> need = rows_needed(p, 1000, 500, 510);
  CHECK(need[0].lo == 395 && need[0].hi == 615 && need[6].lo == 485 && need[6].hi == 525);
  // launches: a separable step gets every present row of its operand, like a convolution
  p.steps = {rank(0, kMedian, 3, B), sep(1, 3, 31, B, 4), table1(2, 5)};
  b = assign_buffers(p);
  const std::vector<Launch> ls = band_launches(p, b, 100, 40, 50, 20, true);
  CHECK(ls.size() == 3 && ls[1].y0 == 40 && ls[1].nrows == 10 && ls[1].src0 == 25 && ls[1].nsrc == 40);
  CHECK(ls[1].a_row == 5 && ls[1].dst_row == 20 && ls[1].a_buf != ls[1].dst_buf && ls[2].dst_buf == kOut);
  std::printf("{\"checked\": %d, \"failed\": %d}\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}

// ---- grid: a scalar model of the steps, band by band ----------------------------------------------

struct Val {
  int lo = 0, hi = 0;  // the rows present
  std::vector<uint8_t> d;
};

int g_bad_reads = 0;

struct Frame {
  int W, H;
  size_t row() const { return (size_t)W * 3; }
};

uint8_t at(const Val &v, const Frame &f, int y, int x, int c) {
  if (y < v.lo || y >= v.hi) {  // a row the plan did not say exists
    ++g_bad_reads;
    return 0x5A;
  }
  return v.d[(size_t)(y - v.lo) * f.row() + (size_t)x * 3 + c];
}

int round_shift(int acc, int shift, int rounding) {
  if (shift == 0) return acc;
  const int fl = acc >> shift, r = acc & ((1 << shift) - 1), h = 1 << (shift - 1);
  if (rounding == kRoundHalfUp) return (acc + h) >> shift;
  return fl + ((r > h) || (r == h && (fl & 1)));
}

int floor_div(long n, long d) { return (int)(n >= 0 ? n / d : -((-n + d - 1) / d)); }

Val run_step(const Step &s, const std::vector<Val> &vals, const Frame &f, Rows out) {
  Val o;
  o.lo = out.lo, o.hi = out.hi;
  o.d.assign((size_t)(out.hi - out.lo) * f.row(), 0);
  for (int y = out.lo; y < out.hi; ++y)
    for (int x = 0; x < f.W; ++x)
      for (int c = 0; c < 3; ++c) {
        int r = 0;
        if (s.kind == kTable) {
          r = s.table[at(vals[s.a], f, y, x, c)];
        } else if (s.kind == kBinary) {
          const int a = at(vals[s.a], f, y, x, c), b = at(vals[s.b], f, y, x, c);
          r = s.op == kSubtract ? a - b : s.op == kAdd ? a + b : s.op == kAbsdiff ? std::abs(a - b) : s.op == kMin ? (a < b ? a : b) : (a > b ? a : b);
        } else if (s.kind == kSep) {
          int acc = 0;
          for (int j = 0; j < s.kh; ++j) {
            const int by = vf::conv::border_index(y + j - s.kh / 2, f.H, s.border);  // FRAME coordinates
            if (by < 0) continue;
            int rowsum = 0;
            for (int i = 0; i < s.kw; ++i) {
              const int bx = vf::conv::border_index(x + i - s.kw / 2, f.W, s.border);
              if (bx >= 0) rowsum += s.taps_x[(size_t)i] * at(vals[s.a], f, by, bx, c);
            }
            acc += s.taps_y[(size_t)j] * rowsum;
          }
          r = s.divisor > 1 ? floor_div(2L * acc + s.divisor, 2L * s.divisor) : round_shift(acc, s.shift, s.op);
        } else {  // kRank: erode, dilate, median
          int mn = 255, mx = 0, cnt = 0;
          int med[49];
          for (int j = 0; j < s.kh; ++j)
            for (int i = 0; i < s.kw; ++i) {
              const int by = vf::conv::border_index(y + j - s.kh / 2, f.H, s.border);
              const int bx = vf::conv::border_index(x + i - s.kw / 2, f.W, s.border);
              if (by < 0 || bx < 0) continue;
              const int v = at(vals[s.a], f, by, bx, c);
              mn = v < mn ? v : mn, mx = v > mx ? v : mx;
              med[cnt++] = v;
            }
          if (s.op == kErode) r = mn;
          else if (s.op == kDilate) r = mx;
          else {
            for (int a = 1; a < cnt; ++a)
              for (int b = a; b > 0 && med[b - 1] > med[b]; --b) std::swap(med[b - 1], med[b]);
            r = med[cnt / 2];
          }
        }
        o.d[(size_t)(y - out.lo) * f.row() + (size_t)x * 3 + c] = (uint8_t)(r < 0 ? 0 : r > 255 ? 255 : r);
      }
  return o;
}

// rows [y0, y1) of the program's result from rows [s0, s1) of the frame
Val run_band(const Program &p, const Frame &f, const std::vector<uint8_t> &img, int y0, int y1, int s0, int s1) {
  const std::vector<Rows> need = rows_needed(p, f.H, y0, y1);
  std::vector<Val> vals(p.size() + 1);
  CHECK(need[0].lo >= s0 && need[0].hi <= s1);
  vals[0].lo = need[0].lo, vals[0].hi = need[0].hi;
  vals[0].d.assign(img.begin() + (size_t)need[0].lo * f.row(), img.begin() + (size_t)need[0].hi * f.row());
  for (int i = 1; i <= p.size(); ++i) {
    CHECK(need[i].lo >= s0 && need[i].lo < need[i].hi && need[i].hi <= s1);
    vals[i] = run_step(p.steps[i - 1], vals, f, need[i]);
  }
  return vals[p.size()];
}

int run_grid() {
  int cases = 0, multi_band = 0, bands_run = 0;
  unsigned seed = 2107;
  for (int which = 0; which < 3; ++which)
    for (int border = 0; border < 3; ++border) {
      Program p;
      int want_reach;
      if (which == 0) {  // two in a row: 5 x 31 then a 9 x 5 mean, R = 15 + 2
        p.steps = {sep(0, 5, 31, border, 5), sep(1, 9, 5, border, 0, 45)};
        want_reach = 17;
      } else if (which == 1) {  // one feeding a binary step whose other operand is the frame: R = 7
        p.steps = {sep(0, 3, 15, border, 4, 1, kRoundHalfUp), bin(kAbsdiff, 1, 0)};
        want_reach = 7;
      } else {  // one between a rank and a table: R = 1 + 4
        p.steps = {rank(0, kMedian, 3, vf::conv::kReplicate), sep(1, 31, 9, border, 0, 279), table1(2, 5)};
        want_reach = 5;
      }
      std::string why;
      CHECK(validate(p, 3, &why));
      const int R = reach(p);
      CHECK(R == want_reach);
      for (int H : {1, 2, 9, 40, 70})
        for (int W : {1, 4}) {
          const Frame f{W, H};
          std::vector<uint8_t> img((size_t)H * f.row());
          for (uint8_t &b : img) b = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
          const Val whole = run_band(p, f, img, 0, H, 0, H);
          CHECK(whole.lo == 0 && whole.hi == H);
          const int need_rows = 2 * R + 1 < H ? 2 * R + 1 : H;
          for (int rows = need_rows; rows <= H + 1; ++rows) {  // every capacity from 2 R + 1 rows up
            std::vector<vf::conv::Band> bs;
            ++cases;
            CHECK(vf::conv::bands(W, H, 3, R, (size_t)rows * f.row(), &bs));
            multi_band += bs.size() > 1;
            int next = 0;
            for (const vf::conv::Band &b : bs) {
              CHECK(b.y0 == next && b.y1 > b.y0);
              next = b.y1;
              const Val got = run_band(p, f, img, b.y0, b.y1, b.s0, b.s1);
              ++bands_run;
              CHECK(got.lo == b.y0 && got.hi == b.y1);
              CHECK(std::memcmp(got.d.data(), whole.d.data() + (size_t)b.y0 * f.row(), got.d.size()) == 0);
            }
            CHECK(next == H);
          }
        }
    }
  CHECK(g_bad_reads == 0);
  std::printf("{\"cases\": %d, \"multi_band\": %d, \"bands\": %d, \"bad_reads\": %d, \"failed\": %d}\n", cases, multi_band,
              bands_run, g_bad_reads, g_failed);
  return g_failed ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
  const char *mode = argc > 1 ? argv[1] : "";
  if (!std::strcmp(mode, "validate")) return run_validate();
  if (!std::strcmp(mode, "plan")) return run_plan();
  if (!std::strcmp(mode, "grid")) return run_grid();
  std::fprintf(stderr, "usage: chain_plan_sep_check validate | plan | grid\n");
  return 2;
}
