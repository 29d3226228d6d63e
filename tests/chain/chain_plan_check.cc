// chain_plan_check.cc — csrc/vf_chain_plan.h on the CPU (tests/test_chain_plan.py builds this with
// -fsanitize=address,undefined and reads the JSON line it prints).
//   validate   every kind of invalid program is refused with its reason, the valid ones pass
//   fold       a composed table equals the tables in sequence; what must not fold does not
//   buffers    the schedule simulated: no live value overwritten, no neighbourhood step writes its
//              source, the result buffer reported, the count within live values + 1
//   grid       a scalar model of each step run band by band (vf_conv_bands.h with ry = R), reading
//              only rows the plan says exist, borders in frame coordinates, equals the whole frame
//   random     seeded programs over the whole step space (oblong sides, a border per step, a == b,
//              shared tables): validate accepts, fold keeps the picture, the schedule holds, and the
//              library's own launch list (band_launches, what run_launches walks) run on byte buffers
//              equals the whole frame for every capacity from 2 R + 1 rows up, and for the whole frame
//              with the result left in its buffer; a one-step program is one launch with no scratch
//   plan       the reach, the folded steps and the buffers of serialised programs, for the tests that
//              compare them with tests/_chain_ref.py and name features of tests/_chain_gen.py's set
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

int g_failed = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      ++g_failed;                                                  \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);         \
    }                                                              \
  } while (0)

enum { kErode = 0, kDilate = 1, kMedian = 2 };  // VF_RANK_*

Step table1(int a, int seed) {
  Step s;
  s.kind = kTable, s.a = a, s.channels = 1;
  s.table.resize(256);
  for (int v = 0; v < 256; ++v) s.table[v] = (uint8_t)(seed == 0 ? 255 - v : seed == 1 ? (v > 24 ? 255 : 0) : (v * 7 + seed) & 255);
  return s;
}
Step table3(int a) {
  Step s;
  s.kind = kTable, s.a = a, s.channels = 3;
  s.table.resize(768);
  for (int c = 0; c < 3; ++c)
    for (int v = 0; v < 256; ++v) s.table[c * 256 + v] = (uint8_t)((v * (3 + 2 * c) + 11 * c) & 255);
  return s;
}
Step rank(int a, int op, int kw, int kh, int border, bool corner = false) {
  Step s;
  s.kind = kRank, s.a = a, s.op = op, s.kw = kw, s.kh = kh, s.border = border;
  s.element.assign((size_t)kw * kh, corner ? 0 : 1);
  if (corner) s.element[0] = 1;
  return s;
}
Step conv(int a, int k, int border) {  // binomial k x k
  Step s;
  s.kind = kConv, s.a = a, s.kw = k, s.kh = k, s.border = border;
  const int b3[3] = {1, 2, 1}, b5[5] = {1, 4, 6, 4, 1};
  for (int j = 0; j < k; ++j)
    for (int i = 0; i < k; ++i) s.weights.push_back((int16_t)(k == 3 ? b3[j] * b3[i] : b5[j] * b5[i]));
  s.shift = k == 3 ? 4 : 8;
  return s;
}
Step bin(int op, int a, int b) {
  Step s;
  s.kind = kBinary, s.op = op, s.a = a, s.b = b;
  return s;
}

Program edges(int border) {  // median3 -> gradient rect3 -> threshold: R = 2
  Program p;
  p.steps = {rank(0, kMedian, 3, 3, vf::conv::kReplicate), rank(1, kDilate, 3, 3, border), rank(1, kErode, 3, 3, border),
             bin(kSubtract, 2, 3), table1(4, 1)};
  return p;
}
Program blackhat3_it2(int border) {  // subtract(E E D D x, x): R = 4, 5 steps
  Program p;
  p.steps = {rank(0, kDilate, 3, 3, border), rank(1, kDilate, 3, 3, border), rank(2, kErode, 3, 3, border),
             rank(3, kErode, 3, 3, border), bin(kSubtract, 4, 0)};
  return p;
}
Program diamond(int border) {  // add(erode rect7 x, x): value 0 read with reach 3 and reach 0
  Program p;
  p.steps = {rank(0, kErode, 7, 7, border), bin(kAdd, 1, 0)};
  return p;
}
Program dog(int border) {
  Program p;
  p.steps = {conv(0, 3, border), conv(0, 5, border), bin(kAbsdiff, 1, 2), table1(3, 5)};
  return p;
}
Program pointwise() {
  Program p;
  p.steps = {table1(0, 0), table3(1), table1(2, 0)};
  return p;
}
Program eight(int border) {
  Program p;
  p.steps = {rank(0, kErode, 3, 3, border), rank(1, kDilate, 3, 3, border), bin(kSubtract, 0, 2), table1(3, 9),
             conv(4, 3, border), rank(5, kMedian, 3, 3, vf::conv::kReplicate), bin(kMax, 6, 1), bin(kAdd, 7, 3)};
  return p;
}
Program corner_gradient(int border) {
  Program p;
  p.steps = {rank(0, kDilate, 5, 5, border, true), rank(0, kErode, 5, 5, border, true), bin(kSubtract, 2, 1)};
  return p;
}

// ---- validate ---------------------------------------------------------------------------------------

int g_checked = 0;
void refused(const Program &p, int channels, const char *reason) {
  std::string why;
  ++g_checked;
  const bool ok = validate(p, channels, &why);
  if (ok || why.find(reason) == std::string::npos) {
    ++g_failed;
    std::fprintf(stderr, "expected a refusal with \"%s\", got %s \"%s\"\n", reason, ok ? "valid" : "invalid", why.c_str());
  }
}
void accepted(const Program &p, int channels) {
  std::string why;
  ++g_checked;
  if (!validate(p, channels, &why)) {
    ++g_failed;
    std::fprintf(stderr, "expected valid, got \"%s\"\n", why.c_str());
  }
}

int run_validate() {
  const int B = vf::conv::kConstant;
  for (int ch : {1, 3}) {
    accepted(edges(B), ch), accepted(blackhat3_it2(B), ch), accepted(diamond(B), ch), accepted(dog(B), ch);
    accepted(eight(B), ch), accepted(corner_gradient(B), ch);
  }
  accepted(pointwise(), 3);
  refused(pointwise(), 1, "3-channel table on 1-channel frames");
  Program p;
  refused(p, 3, "empty program");
  p = eight(B);
  p.steps.push_back(table1(8, 0));
  refused(p, 3, "9 steps; at most 8");
  p = diamond(B);
  p.steps[0].a = 1;  // reads itself
  refused(p, 3, "step 1: operand a = 1 is not an earlier value");
  p = diamond(B);
  p.steps[0].a = 2;  // reads a later value
  refused(p, 3, "operand a = 2 is not an earlier value");
  p = diamond(B);
  p.steps[1].b = 2;
  refused(p, 3, "step 2: operand b = 2 is not an earlier value");
  p = diamond(B);
  p.steps[1].a = -1;
  refused(p, 3, "not an earlier value");
  p = diamond(B);
  p.steps[1].a = 0;  // add(x, x): value 1 is dead
  refused(p, 3, "value 1 is read by no step");
  p = edges(B);
  p.steps[3].b = 2;  // subtract(dilate, dilate): the erosion is dead
  refused(p, 3, "value 3 is read by no step");
  p = diamond(B);
  p.steps[1].op = 5;
  refused(p, 3, "unknown binary op 5");
  p = diamond(B);
  p.steps[1].kind = 4;
  refused(p, 3, "unknown kind 4");
  p = diamond(B);
  p.steps[0].kh = 9;
  refused(p, 3, "sides are odd and at most 7");
  p = diamond(B);
  p.steps[0].kw = 4;
  refused(p, 3, "sides are odd and at most 7");
  p = diamond(B);
  p.steps[0].element.pop_back();
  refused(p, 3, "kw x kh entries");
  p = pointwise();
  p.steps[1].channels = 2;
  refused(p, 3, "a table has 1 or 3 channels");
  p = pointwise();
  p.steps[0].table.resize(100);
  refused(p, 3, "channels x 256 bytes");
  refused(diamond(B), 2, "frames have 1 or 3 channels");
  // a step's b is not an operand unless the step is binary: any b passes for the others
  p = diamond(B);
  p.steps[0].b = 77;
  accepted(p, 3);
  std::printf("{\"checked\": %d, \"failed\": %d}\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}

// ---- fold -------------------------------------------------------------------------------------------

uint8_t through(const Step &t, int c, uint8_t v) { return t.table[(t.channels == 3 ? 256 * c : 0) + v]; }

int run_fold() {
  const int B = vf::conv::kConstant;
  int tables = 0;
  {  // invert -> 3-channel curves -> invert: one 3-channel table, equal to the sequence
    const Program p = pointwise(), f = fold(p);
    CHECK(f.size() == 1 && f.steps[0].kind == kTable && f.steps[0].a == 0 && f.steps[0].channels == 3);
    CHECK(single_kind(f) == kTable);
    for (int c = 0; c < 3 && f.size() == 1; ++c)
      for (int v = 0; v < 256; ++v, ++tables)
        CHECK(through(f.steps[0], c, (uint8_t)v) ==
              through(p.steps[2], c, through(p.steps[1], c, through(p.steps[0], c, (uint8_t)v))));
  }
  {  // two 1-channel tables stay 1 channel
    Program p;
    p.steps = {table1(0, 3), table1(1, 4)};
    const Program f = fold(p);
    CHECK(f.size() == 1 && f.steps[0].channels == 1 && f.steps[0].table.size() == 256);
    for (int v = 0; v < 256 && f.size() == 1; ++v, ++tables)
      CHECK(f.steps[0].table[v] == p.steps[1].table[p.steps[0].table[v]]);
  }
  {  // 3-channel then 1-channel
    Program p;
    p.steps = {table3(0), table1(1, 4)};
    const Program f = fold(p);
    CHECK(f.size() == 1 && f.steps[0].channels == 3);
    for (int c = 0; c < 3 && f.size() == 1; ++c)
      for (int v = 0; v < 256; ++v, ++tables)
        CHECK(through(f.steps[0], c, (uint8_t)v) == p.steps[1].table[p.steps[0].table[c * 256 + v]]);
  }
  {  // a table with two readers is kept; the tables after the binary step fold, operands renumbered
    Program p;
    p.steps = {table1(0, 3), table1(1, 4), bin(kAdd, 1, 2), table1(3, 5), table1(4, 0)};
    const Program f = fold(p);
    std::string why;
    CHECK(validate(f, 1, &why));
    CHECK(f.size() == 4 && f.steps[0].kind == kTable && f.steps[1].kind == kTable && f.steps[1].a == 1);
    CHECK(f.steps[2].kind == kBinary && f.steps[2].a == 1 && f.steps[2].b == 2 && f.steps[3].a == 3);
    for (int v = 0; v < 256 && f.size() == 4; ++v, ++tables)
      CHECK(f.steps[3].table[v] == p.steps[4].table[p.steps[3].table[v]]);
    CHECK(single_kind(f) == -1);
  }
  {  // a table read by a neighbourhood step is kept; programs without tables are unchanged
    Program p;
    p.steps = {table1(0, 0), rank(1, kErode, 3, 3, B), table1(2, 0)};
    CHECK(fold(p).size() == 3);
    CHECK(fold(blackhat3_it2(B)).size() == 5 && fold(diamond(B)).size() == 2);
    CHECK(fold(edges(B)).size() == 5 && fold(eight(B)).size() == 8);
    Program one;
    one.steps = {rank(0, kErode, 3, 3, B)};
    CHECK(single_kind(one) == kRank);
    one.steps = {conv(0, 3, B)};
    CHECK(single_kind(one) == kConv);
    one.steps = {bin(kAdd, 0, 0)};
    CHECK(single_kind(one) == -1);
  }
  std::printf("{\"tables\": %d, \"failed\": %d}\n", tables, g_failed);
  return g_failed ? 1 : 0;
}

// ---- buffers ----------------------------------------------------------------------------------------

// The schedule of one program simulated: no live value overwritten, no neighbourhood step writes its
// source, the result buffer reported, the count within live values + 1.
void check_schedule(const Program &p, int *max_count, int *in_place) {
  const int n = p.size();
  const Buffers b = assign_buffers(p);
  CHECK((int)b.of.size() == n + 1 && b.of[0] == 0 && b.result == b.of[n]);
  std::vector<int> last(n + 1, 0);
  for (int i = 1; i <= n; ++i) {
    last[p.steps[i - 1].a] = i;
    if (p.steps[i - 1].kind == kBinary) last[p.steps[i - 1].b] = i;
  }
  last[n] = n + 1;
  std::vector<int> holds(b.count, -1);  // the value each buffer holds
  holds[0] = 0;
  int max_live = 1;
  for (int i = 1; i <= n; ++i) {
    const Step &s = p.steps[i - 1];
    const int k = b.of[i];
    CHECK(k >= 0 && k < b.count);
    if (k < 0 || k >= b.count) break;
    // the operands are where the plan says, not overwritten since
    CHECK(holds[b.of[s.a]] == s.a);
    if (s.kind == kBinary) CHECK(holds[b.of[s.b]] == s.b);
    if (is_neighbourhood(s)) CHECK(k != b.of[s.a]);  // never writes the buffer it reads
    const int u = holds[k];
    if (u >= 0 && last[u] >= i) {  // overwrites a value some step from i on reads: only in place
      CHECK(last[u] == i && !is_neighbourhood(s) && reads(s, u));
      ++*in_place;
    }
    holds[k] = i;
    int live = 1;  // value i and every earlier value still to be read (by step i too)
    for (int v = 0; v < i; ++v) live += last[v] >= i;
    if (live > max_live) max_live = live;
  }
  CHECK(holds[b.result] == n);
  CHECK(b.count <= max_live + 1);
  if (b.count > *max_count) *max_count = b.count;
}

int g_one_step = 0;

// A program of one step is one launch from buffer 0 to the caller's output rows, with no scratch:
// what keeps vf_conv_frames_host and vf_rank_frames_host free of allocations beyond the staging.
void check_one_step(const Program &p, int H) {
  if (p.size() != 1) return;
  ++g_one_step;
  const Buffers bufs = assign_buffers(p);
  CHECK(scratch_buffers(bufs, p, true) == 0);
  CHECK(scratch_buffers(bufs, p, false) == bufs.count - 1);
  const std::vector<Launch> ls = band_launches(p, bufs, H, 0, H, 0, true);
  CHECK(ls.size() == 1);
  if (ls.size() != 1) return;
  const Launch &l = ls[0];
  CHECK(l.step == 1 && l.a_buf == 0 && l.a_row == 0 && l.dst_buf == kOut && l.dst_row == 0);
  CHECK(l.y0 == 0 && l.nrows == H && l.src0 == 0 && l.nsrc == H);
  if (p.steps[0].kind == kBinary) CHECK(l.b_buf == 0 && l.b_row == 0);
}

int run_buffers() {
  const int B = vf::conv::kConstant;
  Program same;
  same.steps = {bin(kAdd, 0, 0), bin(kMax, 1, 1)};
  Program fan;  // value 0 stays live to the end
  fan.steps = {rank(0, kErode, 3, 3, B), rank(0, kDilate, 3, 3, B), conv(0, 3, B), bin(kAdd, 1, 2), bin(kMax, 4, 3),
               bin(kMin, 5, 0)};
  const std::vector<Program> ps = {edges(B),  blackhat3_it2(B), diamond(B),          dog(B), pointwise(), fold(pointwise()),
                                   eight(B), corner_gradient(B), same, fan};
  int programs = 0, max_count = 0, in_place = 0;
  for (const Program &p : ps) {
    ++programs;
    check_schedule(p, &max_count, &in_place);
  }
  CHECK(assign_buffers(blackhat3_it2(B)).count <= 3 && assign_buffers(edges(B)).count <= 3);
  CHECK(assign_buffers(diamond(B)).count == 2 && assign_buffers(fold(pointwise())).count == 1);
  for (int H : {1, 7, 40}) {  // a single filter is a one-step program: one launch, no scratch
    Program one;
    for (const Step &st : {rank(0, kErode, 3, 5, B), rank(0, kMedian, 5, 5, vf::conv::kReplicate), conv(0, 5, B), table1(0, 0), bin(kAdd, 0, 0)}) {
      one.steps = {st};
      check_one_step(one, H);
    }
    check_one_step(fold(pointwise()), H);
  }
  CHECK(g_one_step == 18);
  std::printf("{\"programs\": %d, \"max_count\": %d, \"in_place\": %d, \"failed\": %d}\n", programs, max_count, in_place,
              g_failed);
  return g_failed ? 1 : 0;
}

// ---- grid: a scalar model of the steps, band by band ----------------------------------------------

struct Val {
  int lo = 0, hi = 0;  // the rows present
  std::vector<uint8_t> d;
};

int g_bad_reads = 0;

struct Frame {
  int W, H, C;
  size_t row() const { return (size_t)W * C; }
};

// byte (y, x, c) of a value, y and x already resolved into the frame
uint8_t at(const Val &v, const Frame &f, int y, int x, int c) {
  if (y < v.lo || y >= v.hi) {  // a row the plan did not say exists
    ++g_bad_reads;
    return 0x5A;
  }
  return v.d[(size_t)(y - v.lo) * f.row() + (size_t)x * f.C + c];
}

int round_shift(int acc, int shift) {  // round half to even
  if (shift == 0) return acc;
  const int fl = acc >> shift, r = acc & ((1 << shift) - 1), h = 1 << (shift - 1);
  return fl + ((r > h) || (r == h && (fl & 1)));
}

Val run_step(const Step &s, const std::vector<Val> &vals, const Frame &f, Rows out) {
  Val o;
  o.lo = out.lo, o.hi = out.hi;
  o.d.assign((size_t)(out.hi - out.lo) * f.row(), 0);
  for (int y = out.lo; y < out.hi; ++y)
    for (int x = 0; x < f.W; ++x)
      for (int c = 0; c < f.C; ++c) {
        int r = 0;
        if (s.kind == kTable) {
          r = through(s, c, at(vals[s.a], f, y, x, c));
        } else if (s.kind == kBinary) {
          const int a = at(vals[s.a], f, y, x, c), b = at(vals[s.b], f, y, x, c);
          r = s.op == kSubtract ? a - b : s.op == kAdd ? a + b : s.op == kAbsdiff ? std::abs(a - b) : s.op == kMin ? (a < b ? a : b) : (a > b ? a : b);
        } else {
          int acc = 0, mn = 255, mx = 0, cnt = 0;
          int med[49];
          for (int j = 0; j < s.kh; ++j)
            for (int i = 0; i < s.kw; ++i) {
              if (s.kind == kRank && !s.element[(size_t)j * s.kw + i]) continue;
              const int by = vf::conv::border_index(y + j - s.kh / 2, f.H, s.border);  // FRAME coordinates
              const int bx = vf::conv::border_index(x + i - s.kw / 2, f.W, s.border);
              if (by < 0 || bx < 0) continue;  // constant: reads 0 (conv), left out of the set (rank)
              const int v = at(vals[s.a], f, by, bx, c);
              acc += s.kind == kConv ? v * s.weights[(size_t)j * s.kw + i] : 0;
              mn = v < mn ? v : mn, mx = v > mx ? v : mx;
              med[cnt++] = v;
            }
          if (s.kind == kConv) r = round_shift(acc, s.shift);
          else if (s.op == kErode) r = mn;
          else if (s.op == kDilate) r = mx;
          else {
            for (int a = 1; a < cnt; ++a)
              for (int b = a; b > 0 && med[b - 1] > med[b]; --b) std::swap(med[b - 1], med[b]);
            r = med[cnt / 2];
          }
        }
        o.d[(size_t)(y - out.lo) * f.row() + (size_t)x * f.C + c] = (uint8_t)(r < 0 ? 0 : r > 255 ? 255 : r);
      }
  return o;
}

// rows [y0, y1) of the program's result from rows [s0, s1) of the frame
Val run_band(const Program &p, const Frame &f, const std::vector<uint8_t> &img, int y0, int y1, int s0, int s1) {
  const std::vector<Rows> need = rows_needed(p, f.H, y0, y1);
  std::vector<Val> vals(p.size() + 1);
  CHECK(need[0].lo >= s0 && need[0].hi <= s1);  // the upload covers what value 0 must hold
  vals[0].lo = need[0].lo, vals[0].hi = need[0].hi;
  vals[0].d.assign(img.begin() + (size_t)need[0].lo * f.row(), img.begin() + (size_t)need[0].hi * f.row());
  for (int i = 1; i <= p.size(); ++i) {
    CHECK(need[i].lo >= 0 && need[i].lo < need[i].hi && need[i].hi <= f.H);
    CHECK(need[i].lo >= s0 && need[i].hi <= s1);  // every value fits the band's buffer at the band's row origin
    vals[i] = run_step(p.steps[i - 1], vals, f, need[i]);
  }
  return vals[p.size()];
}

int run_grid() {
  int cases = 0, errors = 0, multi_band = 0, bands_run = 0;
  unsigned seed = 12345;
  for (int which = 0; which < 3; ++which)
    for (int border = 0; border < 3; ++border) {
      const Program p = which == 0 ? edges(border) : which == 1 ? blackhat3_it2(border) : diamond(border);
      const int R = reach(p);
      CHECK(R == (which == 0 ? 2 : which == 1 ? 4 : 3));
      for (int H : {1, 2, 3, 9, 40})
        for (int W : {1, 5})
          for (int C : {1, 3}) {
            const Frame f{W, H, C};
            std::vector<uint8_t> img((size_t)H * f.row());
            for (uint8_t &b : img) b = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
            const Val whole = run_band(p, f, img, 0, H, 0, H);
            CHECK(whole.lo == 0 && whole.hi == H);
            // capacities: from one row short of "one row + halo" up to the whole frame and a bit
            const int need_rows = 2 * R + 1 < H ? 2 * R + 1 : H;
            for (int rows = need_rows - 1; rows <= H + 1; ++rows)
              for (int extra : {0, 1}) {
                if (rows < 0 || (rows == need_rows - 1 && extra)) continue;
                const size_t cap = (size_t)rows * f.row() + (extra ? f.row() - 1 : 0);
                std::vector<vf::conv::Band> bs;
                ++cases;
                if (!vf::conv::bands(W, H, C, R, cap, &bs)) {
                  ++errors;
                  CHECK(bs.empty() && rows < need_rows);  // an error, not an endless list; only below 2R + 1 rows
                  continue;
                }
                CHECK(rows >= need_rows);
                multi_band += bs.size() > 1;
                int next = 0;
                for (const vf::conv::Band &b : bs) {
                  CHECK(b.y0 == next && b.y1 > b.y0);
                  next = b.y1;
                  CHECK((size_t)(b.s1 - b.s0) * f.row() <= cap);
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
  std::printf("{\"cases\": %d, \"errors\": %d, \"multi_band\": %d, \"bands\": %d, \"bad_reads\": %d, \"failed\": %d}\n", cases,
              errors, multi_band, bands_run, g_bad_reads, g_failed);
  return g_failed ? 1 : 0;
}

// rows PROGRAM H y0 y1: the plan's rows of every value, for the tests that name figures
int run_rows(const char *name, int H, int y0, int y1) {
  const int B = vf::conv::kConstant;
  const Program p = !std::strcmp(name, "edges") ? edges(B) : !std::strcmp(name, "blackhat3_it2") ? blackhat3_it2(B) : diamond(B);
  const std::vector<Rows> need = rows_needed(p, H, y0, y1);
  std::printf("{\"reach\": %d, \"rows\": [", reach(p));
  for (size_t v = 0; v < need.size(); ++v) std::printf("%s[%d, %d]", v ? ", " : "", need[v].lo, need[v].hi);
  std::printf("]}\n");
  return 0;
}

// ---- random: seeded programs through validate, fold, the schedule and a buffer-addressed executor ----

struct Lcg {
  unsigned s;
  unsigned next() { return (s = s * 1664525u + 1013904223u) >> 8; }
  int below(int n) { return (int)(next() % (unsigned)n); }  // 0 .. n - 1
  bool chance(int percent) { return below(100) < percent; }
};

// A valid program of 1 .. 8 steps over the whole step space: permutation tables of 1 or (for
// 3-channel frames) 3 channels, kernels and elements with independent odd sides 1 .. 7 and their own
// border, the medians, all five binary ops with a == b for add / min / max.  The operands are steered
// so that every value but the last is read: a step must read `must` values nobody has read yet when
// the steps after it (one unread value fewer each, at best) could not read them all.
Program random_program(Lcg &g, int channels) {
  const int n = 1 + g.below(kMaxSteps);
  Program p;
  std::vector<int> unread{0};
  auto take = [&](int v) {
    for (size_t k = 0; k < unread.size(); ++k)
      if (unread[k] == v) return (void)unread.erase(unread.begin() + (long)k);
  };
  for (int i = 1; i <= n; ++i) {
    const int rem = n - i;
    const int must = (int)unread.size() > rem ? (int)unread.size() - rem : 0;
    auto operand = [&](int avoid) {
      std::vector<int> fresh;
      for (int v : unread)
        if (v != avoid) fresh.push_back(v);
      if (!fresh.empty() && (must || g.chance(70))) return fresh[(size_t)g.below((int)fresh.size())];
      return g.below(i);
    };
    const int kind = must == 2 ? kBinary : g.below(4);
    Step s;
    s.kind = kind;
    s.a = operand(-1);
    if (kind == kTable) {
      s.channels = channels == 3 && g.chance(50) ? 3 : 1;
      s.table.resize((size_t)s.channels * 256);
      for (int c = 0; c < s.channels; ++c) {  // a permutation: Fisher-Yates
        uint8_t *t = s.table.data() + 256 * c;
        for (int v = 0; v < 256; ++v) t[v] = (uint8_t)v;
        for (int v = 255; v > 0; --v) std::swap(t[v], t[g.below(v + 1)]);
      }
    } else if (kind == kConv) {
      s.kh = 1 + 2 * g.below(4), s.kw = 1 + 2 * g.below(4), s.border = g.below(3), s.shift = g.below(9);
      const int m = g.chance(25) ? 8 + g.below(33) : 1 + g.below(3);
      int sum = 0;
      for (int k = 0; k < s.kw * s.kh; ++k) s.weights.push_back((int16_t)(g.below(2 * m + 1) - m)), sum += s.weights.back();
      int16_t &centre = s.weights[(size_t)(s.kh / 2) * s.kw + s.kw / 2];
      centre = (int16_t)(centre + (1 << s.shift) - sum);  // unit gain
    } else if (kind == kRank) {
      if (g.chance(25)) {
        s.op = kMedian, s.kw = s.kh = g.chance(50) ? 3 : 5, s.border = vf::conv::kReplicate;
        s.element.assign((size_t)s.kw * s.kh, 1);
      } else {
        s.op = g.below(2), s.kh = 1 + 2 * g.below(4), s.kw = 1 + 2 * g.below(4), s.border = g.below(3);
        bool any = false;
        for (int k = 0; k < s.kw * s.kh; ++k) s.element.push_back((uint8_t)g.below(2)), any |= s.element.back() != 0;
        if (!any) s.element[(size_t)g.below(s.kw * s.kh)] = 1;
      }
    } else {
      if (must < 2 && (i == 1 || g.chance(30))) {
        const int same[3] = {kAdd, kMin, kMax};
        s.op = same[g.below(3)], s.b = s.a;
      } else {
        s.op = g.below(5);
        s.b = operand(s.a);
        while (s.b == s.a) s.b = g.below(i);
        if (g.chance(50)) std::swap(s.a, s.b);
      }
    }
    take(s.a);
    if (kind == kBinary) take(s.b);
    unread.push_back(i);
    p.steps.push_back(std::move(s));
  }
  return p;
}

int g_in_place_run = 0, g_launches = 0;

// Rows [b.y0, b.y1) of the (folded) program's result by the library's own addressing: the launches
// of band_launches(), walked as run_launches (vf_api.hip) walks them.  One byte buffer per
// buffer the launches may address (1 + scratch_buffers), each of the band's source rows [b.s0, b.s1);
// buffer 0 starts as the upload.  Every buffer index, row offset, src0 and nsrc comes from the
// Launch.  A table or binary step reads and writes byte by byte, in place where its Launch names one
// buffer row for operand and result; a neighbourhood step resolves a tap in frame coordinates and
// then moves it into the window [src0, src0 + nsrc) that starts at the operand's a_row.  tag[k][row]
// is the value and the frame row a buffer row holds: a read of a row that does not hold that row of
// the operand, or an address outside a buffer, is a bad read.  With result_to_out (the raw path's
// form) the last step writes the output rows; without (the codec's) the result is read back from
// its planned buffer.
std::vector<uint8_t> run_band_buffers(const Program &p, const Frame &f, const std::vector<uint8_t> &img,
                                      const vf::conv::Band &b, bool result_to_out) {
  const int n = p.size();
  const Buffers bufs = assign_buffers(p);
  const std::vector<Launch> ls = band_launches(p, bufs, f.H, b.y0, b.y1, b.s0, result_to_out);
  const size_t row = f.row();
  const int buf_rows = b.s1 - b.s0, nbuf = 1 + scratch_buffers(bufs, p, result_to_out);
  struct Tag {
    int value = -1, y = -1;
  };
  std::vector<std::vector<uint8_t>> buf((size_t)nbuf, std::vector<uint8_t>((size_t)buf_rows * row, 0x5A));
  std::vector<std::vector<Tag>> tag((size_t)nbuf, std::vector<Tag>((size_t)buf_rows));
  std::memcpy(buf[0].data(), img.data() + (size_t)b.s0 * row, (size_t)buf_rows * row);
  for (int r = 0; r < buf_rows; ++r) tag[0][(size_t)r] = Tag{0, b.s0 + r};
  std::vector<uint8_t> out((size_t)(b.y1 - b.y0) * row, 0xA5);
  CHECK(nbuf <= bufs.count && (result_to_out || nbuf == bufs.count));
  CHECK((int)ls.size() == n);
  // rows [r, r + count) of buffer k lie inside the buffers
  auto inside = [&](int k, int r, int count) { return k >= 0 && k < nbuf && count > 0 && r >= 0 && r + count <= buf_rows; };
  // byte `off` of row r of buffer k, which must hold row y of value v
  auto load = [&](int v, int y, int k, int r, size_t off) -> uint8_t {
    if (!inside(k, r, 1) || tag[(size_t)k][(size_t)r].value != v || tag[(size_t)k][(size_t)r].y != y) {
      ++g_bad_reads;
      return 0x5A;
    }
    return buf[(size_t)k][(size_t)r * row + off];
  };
  for (size_t li = 0; li < ls.size(); ++li) {
    const Launch &l = ls[li];
    ++g_launches;
    CHECK(l.step == (int)li + 1);
    if (l.step < 1 || l.step > n) return out;
    const Step &s = p.steps[(size_t)l.step - 1];
    const bool to_out = l.dst_buf == kOut;
    CHECK(to_out == (result_to_out && l.step == n));
    // every (buffer, row) the launch names lies inside 1 + scratch_buffers buffers of s1 - s0 rows
    const bool addressed = inside(l.a_buf, l.a_row, l.nsrc) && (s.kind != kBinary || inside(l.b_buf, l.b_row, l.nrows)) &&
                           (to_out ? l.dst_row == 0 && l.y0 == b.y0 && l.nrows == b.y1 - b.y0 : inside(l.dst_buf, l.dst_row, l.nrows));
    CHECK(addressed);
    if (!addressed) return out;
    CHECK(is_neighbourhood(s) || l.nsrc == l.nrows);
    if (!to_out && (l.dst_buf == l.a_buf || (s.kind == kBinary && l.dst_buf == l.b_buf))) {
      CHECK(!is_neighbourhood(s));  // a neighbourhood step never runs in place
      CHECK(l.dst_row == (l.dst_buf == l.a_buf ? l.a_row : l.b_row));  // in place is dst == operand exactly
      ++g_in_place_run;
    }
    for (int yy = 0; yy < l.nrows; ++yy) {
      const int y = l.y0 + yy;
      for (size_t off = 0; off < row; ++off) {
        const int x = (int)(off / (size_t)f.C), c = (int)(off % (size_t)f.C);
        int q = 0;
        if (s.kind == kTable) {
          q = through(s, c, load(s.a, y, l.a_buf, l.a_row + yy, off));
        } else if (s.kind == kBinary) {
          const int a = load(s.a, y, l.a_buf, l.a_row + yy, off), bb = load(s.b, y, l.b_buf, l.b_row + yy, off);
          q = s.op == kSubtract ? a - bb : s.op == kAdd ? a + bb : s.op == kAbsdiff ? std::abs(a - bb) : s.op == kMin ? (a < bb ? a : bb) : (a > bb ? a : bb);
        } else {
          int acc = 0, mn = 255, mx = 0, cnt = 0;
          int med[49];
          for (int j = 0; j < s.kh; ++j)
            for (int t = 0; t < s.kw; ++t) {
              if (s.kind == kRank && !s.element[(size_t)j * s.kw + t]) continue;
              const int by = vf::conv::border_index(y + j - s.kh / 2, f.H, s.border);
              const int bx = vf::conv::border_index(x + t - s.kw / 2, f.W, s.border);
              if (by < 0 || bx < 0) continue;
              const int sr = by - l.src0;  // launch_conv / launch_rank's s0 and nsrc
              int v = 0x5A;
              if (sr < 0 || sr >= l.nsrc) ++g_bad_reads;  // the kernel would stage a neutral value here
              else v = load(s.a, by, l.a_buf, l.a_row + sr, (size_t)bx * f.C + c);
              acc += s.kind == kConv ? v * s.weights[(size_t)j * s.kw + t] : 0;
              mn = v < mn ? v : mn, mx = v > mx ? v : mx;
              med[cnt++] = v;
            }
          if (s.kind == kConv) q = round_shift(acc, s.shift);
          else if (s.op == kErode) q = mn;
          else if (s.op == kDilate) q = mx;
          else {
            for (int a = 1; a < cnt; ++a)
              for (int bb = a; bb > 0 && med[bb - 1] > med[bb]; --bb) std::swap(med[bb - 1], med[bb]);
            q = med[cnt / 2];
          }
        }
        const uint8_t byte = (uint8_t)(q < 0 ? 0 : q > 255 ? 255 : q);
        if (to_out) out[(size_t)(l.dst_row + yy) * row + off] = byte;
        else buf[(size_t)l.dst_buf][(size_t)(l.dst_row + yy) * row + off] = byte;
      }
      if (!to_out) tag[(size_t)l.dst_buf][(size_t)(l.dst_row + yy)] = Tag{l.step, y};
    }
  }
  if (!result_to_out)  // the encoder's read: the result's rows from the buffer the plan reports
    for (int y = b.y0; y < b.y1; ++y)
      for (size_t off = 0; off < row; ++off)
        out[(size_t)(y - b.y0) * row + off] = load(n, y, bufs.result, y - b.s0, off);
  return out;
}

bool has_table3(const Program &p) {
  for (const Step &s : p.steps)
    if (s.kind == kTable && s.channels == 3) return true;
  return false;
}

int run_random(int count) {
  Lcg g{20240607u};
  int programs = 0, cases = 0, multi_band = 0, bands_run = 0, folded = 0, max_count = 0, in_place = 0, max_reach = 0;
  int oblong = 0, one_row = 0, codec_form = 0;
  for (int k = 0; k < count; ++k) {
    const int channels = k & 1 ? 3 : 1;
    const Program p = random_program(g, channels);
    ++programs;
    std::string why;
    const bool valid = validate(p, channels, &why);
    if (!valid) std::fprintf(stderr, "program %d refused: %s\n", k, why.c_str());
    CHECK(valid);
    if (!valid) continue;
    const Program fp = fold(p);
    CHECK(validate(fp, channels, &why));
    folded += fp.size() < p.size();
    check_schedule(p, &max_count, &in_place);
    check_schedule(fp, &max_count, &in_place);
    const int R = reach(fp);
    CHECK(R == reach(p));  // a table has no radius: folding moves no row
    if (R > max_reach) max_reach = R;
    for (const Step &s : p.steps) oblong += is_neighbourhood(s) && s.kw != s.kh, one_row += is_neighbourhood(s) && s.kh == 1 && s.kw > 1;
    for (int H : {1, 2, 9, 40})
      for (int W : {1, 5})
        for (int C : {1, 3}) {
          if (C == 1 && has_table3(p)) continue;
          const Frame f{W, H, C};
          std::vector<uint8_t> img((size_t)H * f.row());
          for (uint8_t &b : img) b = (uint8_t)(g.next() >> 8);
          // the whole frame by the scalar model of the program as written, every value its own vector
          const Val whole = run_band(p, f, img, 0, H, 0, H);
          const Val whole_folded = run_band(fp, f, img, 0, H, 0, H);
          CHECK(whole.d == whole_folded.d);
          // the codec's form: the whole frame at once, the result left in its planned buffer
          const bool codec_same = run_band_buffers(fp, f, img, vf::conv::Band{0, H, 0, H}, false) == whole.d;
          if (!codec_same && g_failed < 20)
            std::fprintf(stderr, "program %d, %d x %d x %d: the whole frame with the result in its buffer differs\n", k, W, H, C);
          CHECK(codec_same);
          ++codec_form;
          check_one_step(fp, H);
          const int need_rows = 2 * R + 1 < H ? 2 * R + 1 : H;
          for (int rows = need_rows; rows <= H + 1; ++rows) {
            std::vector<vf::conv::Band> bs;
            ++cases;
            const bool cut = vf::conv::bands(W, H, C, R, (size_t)rows * f.row(), &bs);
            CHECK(cut);
            if (!cut) continue;
            multi_band += bs.size() > 1;
            int next = 0;
            for (const vf::conv::Band &b : bs) {
              CHECK(b.y0 == next && b.y1 > b.y0 && b.s1 - b.s0 <= rows);
              next = b.y1;
              const std::vector<uint8_t> got = run_band_buffers(fp, f, img, b, true);
              ++bands_run;
              const bool same = std::memcmp(got.data(), whole.d.data() + (size_t)b.y0 * f.row(), got.size()) == 0;
              if (!same && g_failed < 20)
                std::fprintf(stderr, "program %d, %d x %d x %d, %d rows fit: rows [%d, %d) from [%d, %d) differ\n", k, W, H, C,
                             rows, b.y0, b.y1, b.s0, b.s1);
              CHECK(same);
            }
            CHECK(next == H);
          }
        }
  }
  CHECK(g_bad_reads == 0);
  std::printf("{\"programs\": %d, \"cases\": %d, \"multi_band\": %d, \"bands\": %d, \"folded\": %d, \"max_count\": %d, "
              "\"in_place\": %d, \"in_place_run\": %d, \"max_reach\": %d, \"oblong\": %d, \"one_row\": %d, \"codec_form\": %d, "
              "\"one_step\": %d, \"launches\": %d, \"bad_reads\": %d, \"failed\": %d}\n",
              programs, cases, multi_band, bands_run, folded, max_count, in_place, g_in_place_run, max_reach, oblong, one_row,
              codec_form, g_one_step, g_launches, g_bad_reads, g_failed);
  return g_failed ? 1 : 0;
}

// plan FILE: the plan of each serialised program (tests/_chain_gen.py's serialise: the structure,
// no contents): its reach, the folded program's steps as [kind, a, b, op], its buffers and the result's.
int run_plan(const char *path) {
  std::FILE *fp = std::fopen(path, "r");
  if (!fp) return 2;
  std::printf("[");
  int n = 0, channels = 0, count = 0;
  char tagc = 0;
  while (std::fscanf(fp, " %c %d %d", &tagc, &n, &channels) == 3 && tagc == 'P') {
    Program p;
    for (int i = 0; i < n; ++i) {
      Step s;
      int tch = 1;
      if (std::fscanf(fp, "%d %d %d %d %d %d %d", &s.kind, &s.a, &s.b, &s.op, &s.kw, &s.kh, &tch) != 7) return std::fclose(fp), 2;
      if (s.kind == kTable) s.channels = tch, s.table.assign((size_t)(tch == 3 ? 3 : 1) * 256, 0);
      if (s.kind == kConv && s.kw > 0 && s.kh > 0) s.weights.assign((size_t)s.kw * s.kh, 1);
      if (s.kind == kRank && s.kw > 0 && s.kh > 0) s.element.assign((size_t)s.kw * s.kh, 1);
      p.steps.push_back(std::move(s));
    }
    std::string why;
    const bool valid = validate(p, channels, &why);
    const Program f = valid ? fold(p) : p;
    const Buffers b = valid ? assign_buffers(f) : Buffers();
    std::printf("%s{\"valid\": %s, \"reach\": %d, \"steps\": [", count++ ? ", " : "", valid ? "true" : "false", valid ? reach(p) : -1);
    for (int i = 0; valid && i < f.size(); ++i)
      std::printf("%s[%d, %d, %d, %d]", i ? ", " : "", f.steps[i].kind, f.steps[i].a,
                  f.steps[i].kind == kBinary ? f.steps[i].b : -1, f.steps[i].op);
    std::printf("], \"of\": [");
    for (size_t v = 0; v < b.of.size(); ++v) std::printf("%s%d", v ? ", " : "", b.of[v]);
    std::printf("], \"count\": %d, \"result\": %d}", b.count, b.result);
  }
  std::fclose(fp);
  std::printf("]\n");
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "validate") return run_validate();
  if (mode == "fold") return run_fold();
  if (mode == "buffers") return run_buffers();
  if (mode == "grid") return run_grid();
  if (mode == "rows" && argc == 6) return run_rows(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
  if (mode == "random") return run_random(argc > 2 ? std::atoi(argv[2]) : 500);
  if (mode == "plan" && argc == 3) return run_plan(argv[2]);
  std::fprintf(stderr, "usage: chain_plan_check validate | fold | buffers | grid | rows PROGRAM H y0 y1 | random [N] | plan FILE\n");
  return 2;
}
