// chain_plan_mix_check — csrc/vf_chain_plan.h's colour-matrix step (kind 5) on the CPU.  Modes:
//   validate   kind 5 is accepted on 3 channels and refused on 1; kind 4 stays "unknown kind 4"
//   plan       in-place placement, no fold across a mix, single_kind, radius 0
//   grid       a scalar model of the steps, band by band on only the rows the plan says exist,
//              equals the whole frame for a program with a mix between two neighbourhood steps
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
Step conv3(int a, int border) {  // binomial 3 x 3 / 16
  Step s;
  s.kind = kConv, s.a = a, s.kw = 3, s.kh = 3, s.border = border, s.shift = 4;
  const int b3[3] = {1, 2, 1};
  for (int j = 0; j < 3; ++j)
    for (int i = 0; i < 3; ++i) s.weights.push_back((int16_t)(b3[j] * b3[i]));
  return s;
}
Step bin(int op, int a, int b) {
  Step s;
  s.kind = kBinary, s.op = op, s.a = a, s.b = b;
  return s;
}
Step mix(int a, int rounding = kRoundHalfEven) {  // a luma-like row, a negative weight, an offset: shift 4
  Step s;
  s.kind = kMix, s.a = a, s.op = rounding, s.shift = 4;
  s.matrix = {2, 9, 5, 8, 20, -3, -1, -40, 1, 1, 30, 7};
  return s;
}

bool refused(const Program &p, int channels, const char *reason) {
  std::string why;
  return !validate(p, channels, &why) && why.find(reason) != std::string::npos;
}

int run_validate() {
  Program p;
  p.steps = {mix(0)};
  std::string why;
  CHECK(validate(p, 3, &why));
  CHECK(refused(p, 1, "step 1: a colour matrix on 1-channel frames"));
  p.steps = {rank(0, kMedian, 3, vf::conv::kReplicate), mix(1, kRoundHalfUp), table1(2, 3)};
  CHECK(validate(p, 3, &why));
  CHECK(refused(p, 1, "step 2: a colour matrix on 1-channel frames"));
  p.steps = {mix(0)};
  p.steps[0].kind = 4;  // the gap: not a kind
  CHECK(refused(p, 3, "step 1: unknown kind 4"));
  CHECK(refused(p, 1, "step 1: unknown kind 4"));
  for (int k : {-1, 6, 9}) {
    p.steps[0].kind = k;
    CHECK(refused(p, 3, ("unknown kind " + std::to_string(k)).c_str()));
  }
  p.steps = {mix(0)};
  p.steps[0].op = 2;
  CHECK(refused(p, 3, "unknown rounding 2"));
  p.steps = {mix(0)};
  p.steps[0].matrix.pop_back();
  CHECK(refused(p, 3, "3 x 4"));
  p.steps = {mix(1)};  // operands as for every step
  CHECK(refused(p, 3, "operand a = 1 is not an earlier value"));
  p.steps = {mix(0), mix(0)};
  CHECK(refused(p, 3, "value 1 is read by no step"));
  CHECK(kMix == 5 && kTable == 0 && kConv == 1 && kRank == 2 && kBinary == 3);
  std::printf("{\"checked\": %d, \"failed\": %d}\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}

int run_plan() {
  const int B = vf::conv::kReplicate;
  Program p;
  // a mix over an operand that dies there is placed in place
  p.steps = {rank(0, kMedian, 3, B), mix(1), rank(2, kErode, 3, B)};
  Buffers b = assign_buffers(p);
  CHECK(b.of[1] != b.of[0] && b.of[2] == b.of[1] && b.of[3] != b.of[2]);
  CHECK(reach(p) == 2 && radius(p.steps[1]) == 0 && !is_neighbourhood(p.steps[1]));
  p.steps = {mix(0)};  // value 0 dies at step 1: over the upload itself
  b = assign_buffers(p);
  CHECK(b.of[1] == 0 && b.count == 1 && b.result == 0);
  CHECK(single_kind(p) == kMix && single_kind(fold(p)) == kMix);
  CHECK(scratch_buffers(b, p, true) == 0);
  // an operand that is read later keeps its buffer: the mix may not run in place
  p.steps = {mix(0), bin(kAbsdiff, 1, 0)};
  b = assign_buffers(p);
  CHECK(b.of[1] != b.of[0]);
  CHECK(b.of[2] == b.of[1] || b.of[2] == b.of[0]);  // the binary step is in place over one of them
  CHECK(single_kind(p) == -1);
  // no fold across a mix: table -> mix -> table stays 3 steps, mix -> mix stays 2
  p.steps = {table1(0, 0), mix(1), table1(2, 5)};
  Program f = fold(p);
  CHECK(f.size() == 3 && f.steps[0].kind == kTable && f.steps[1].kind == kMix && f.steps[2].kind == kTable);
  CHECK(f.steps[1].a == 1 && f.steps[2].a == 2 && f.steps[1].matrix == p.steps[1].matrix && f.steps[1].shift == 4);
  p.steps = {mix(0), mix(1, kRoundHalfUp)};
  f = fold(p);
  CHECK(f.size() == 2 && f.steps[1].op == kRoundHalfUp);
  p.steps = {table1(0, 0), table1(1, 5), mix(2), table1(3, 7), table1(4, 0)};  // the tables on each side still fold
  f = fold(p);
  CHECK(f.size() == 3 && f.steps[1].kind == kMix && f.steps[1].a == 1 && f.steps[2].a == 2);
  // launches: a mix reads its operand at its own first row, like a table
  p.steps = {rank(0, kMedian, 3, B), mix(1), rank(2, kErode, 3, B)};
  b = assign_buffers(p);
  const std::vector<Launch> ls = band_launches(p, b, 40, 10, 20, 8, true);
  CHECK(ls.size() == 3 && ls[1].y0 == 9 && ls[1].nrows == 12 && ls[1].a_row == 1 && ls[1].dst_row == 1);
  CHECK(ls[1].a_buf == ls[1].dst_buf && ls[2].dst_buf == kOut);
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
        } else if (s.kind == kMix) {
          int acc = s.matrix[4 * c + 3];
          for (int k = 0; k < 3; ++k) acc += s.matrix[4 * c + k] * at(vals[s.a], f, y, x, k);
          r = round_shift(acc, s.shift, s.op);
        } else if (s.kind == kBinary) {
          const int a = at(vals[s.a], f, y, x, c), b = at(vals[s.b], f, y, x, c);
          r = s.op == kSubtract ? a - b : s.op == kAdd ? a + b : s.op == kAbsdiff ? std::abs(a - b) : s.op == kMin ? (a < b ? a : b) : (a > b ? a : b);
        } else {
          int acc = 0, mn = 255, mx = 0, cnt = 0;
          int med[49];
          for (int j = 0; j < s.kh; ++j)
            for (int i = 0; i < s.kw; ++i) {
              const int by = vf::conv::border_index(y + j - s.kh / 2, f.H, s.border);  // FRAME coordinates
              const int bx = vf::conv::border_index(x + i - s.kw / 2, f.W, s.border);
              if (by < 0 || bx < 0) continue;
              const int v = at(vals[s.a], f, by, bx, c);
              acc += s.kind == kConv ? v * s.weights[(size_t)j * s.kw + i] : 0;
              mn = v < mn ? v : mn, mx = v > mx ? v : mx;
              med[cnt++] = v;
            }
          if (s.kind == kConv) r = round_shift(acc, s.shift, kRoundHalfEven);
          else if (s.op == kErode) r = mn;
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
  unsigned seed = 2005;
  for (int which = 0; which < 2; ++which)
    for (int border = 0; border < 3; ++border) {
      Program p;
      if (which == 0)  // gray-like -> median -> gradient: a mix between neighbourhood steps, R = 3
        p.steps = {conv3(0, border), mix(1), rank(2, kMedian, 3, vf::conv::kReplicate), rank(3, kDilate, 3, border),
                   rank(3, kErode, 3, border), bin(kSubtract, 4, 5)};
      else  // the mix's operand is read again: absdiff(erode(mix(conv x)), conv x), R = 2
        p.steps = {conv3(0, border), mix(1, kRoundHalfUp), rank(2, kErode, 3, border), bin(kAbsdiff, 3, 1)};
      std::string why;
      CHECK(validate(p, 3, &why));
      const int R = reach(p);
      CHECK(R == (which == 0 ? 3 : 2));
      for (int H : {1, 2, 9, 40})
        for (int W : {1, 5}) {
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
  std::fprintf(stderr, "usage: chain_plan_mix_check validate | plan | grid\n");
  return 2;
}
