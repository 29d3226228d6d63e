// chain_plan_level_check — csrc/vf_chain_plan.h's level step (kind 8) on the CPU.  Modes:
//   validate   kind 8 is accepted on 1 and 3 channels and its bad arguments are refused with the
//              level filter's own words; kinds 4, 6, 9 and -1 stay "unknown kind N"
//   plan       a level step over a dying operand is placed in place; nothing folds across one;
//              single_kind reports it; whole_frame; its radius and a program's reach do not grow;
//              rows_needed and band_launches give whole frames for every value of a program that
//              holds one, whatever rows are asked for, and bands as before for one that does not
// Each prints one JSON line; exit status 1 when a check failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vf_chain_plan.h"
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

Step table1(int a, int seed) {
  Step s;
  s.kind = kTable, s.a = a, s.channels = 1;
  s.table.resize(256);
  for (int v = 0; v < 256; ++v) s.table[v] = (uint8_t)(seed == 0 ? 255 - v : (v * 7 + seed) & 255);
  return s;
}
Step rank(int a, int k) {
  Step s;
  s.kind = kRank, s.a = a, s.op = 0, s.kw = k, s.kh = k, s.border = vf::conv::kReplicate;
  s.element.assign((size_t)k * k, 1);
  return s;
}
Step bin(int op, int a, int b) {
  Step s;
  s.kind = kBinary, s.op = op, s.a = a, s.b = b;
  return s;
}
Step mix(int a) {
  Step s;
  s.kind = kMix, s.a = a, s.op = kRoundHalfEven, s.shift = 0;
  s.matrix = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  return s;
}
Step level(int a, int rule = vf::level::kEqualize, int mask = 0, int link = 0, int lo = 0, int hi = 0) {
  Step s;
  s.kind = kLevel, s.a = a, s.op = rule, s.mask = mask, s.link = link, s.clip_lo = lo, s.clip_hi = hi;
  return s;
}

bool refused(const Program &p, int channels, const char *reason) {
  std::string why;
  return !validate(p, channels, &why) && why.find(reason) != std::string::npos;
}

int run_validate() {
  Program p;
  std::string why;
  CHECK(kLevel == 8 && kSep == 7 && kMix == 5 && kTable == 0 && kConv == 1 && kRank == 2 && kBinary == 3);
  for (int ch : {1, 3})
    for (int rule : {0, 1})
      for (int link : {0, 1}) {
        p.steps = {level(0, rule, 0, link, 0, 0)};
        CHECK(validate(p, ch, &why));
        p.steps = {level(0, rule, 1, link, 0, 0)};
        CHECK(validate(p, ch, &why));
      }
  for (int mask = 0; mask < 8; ++mask) {
    p.steps = {level(0, 1, mask, 1, 655, 32767)};
    CHECK(validate(p, 3, &why));
  }
  p.steps = {level(0, 0, 2)};
  CHECK(refused(p, 1, "step 1: channel mask 2 names a channel beyond the frame's 1"));
  p.steps = {level(0, 0, 8)};
  CHECK(refused(p, 3, "step 1: channel mask 8 outside 0..7"));
  p.steps = {level(0, 2)};
  CHECK(refused(p, 3, "step 1: unknown level rule 2"));
  p.steps = {level(0, 0, 0, 2)};
  CHECK(refused(p, 3, "step 1: link=2 is not 0 or 1"));
  p.steps = {level(0, 1, 0, 0, 32768, 0)};
  CHECK(refused(p, 3, "step 1: clips 32768, 0 outside 0..32767"));
  p.steps = {level(0, 0, 0, 0, 0, 7)};
  CHECK(refused(p, 1, "step 1: the equalize rule takes no clips"));
  p.steps = {table1(0, 1), level(1, 0, 4)};
  CHECK(refused(p, 1, "step 2: channel mask 4 names a channel"));
  for (int k : {4, 6, 9, -1}) {  // not kinds
    p.steps = {level(0)};
    p.steps[0].kind = k;
    CHECK(refused(p, 3, ("step 1: unknown kind " + std::to_string(k)).c_str()));
    CHECK(refused(p, 1, ("step 1: unknown kind " + std::to_string(k)).c_str()));
  }
  p.steps = {level(1)};  // operands as for every step
  CHECK(refused(p, 3, "operand a = 1 is not an earlier value"));
  p.steps = {level(0), level(0)};
  CHECK(refused(p, 3, "value 1 is read by no step"));
  std::printf("{\"checked\": %d, \"failed\": %d}\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}

bool whole(const std::vector<Rows> &r, int H) {
  for (const Rows &x : r)
    if (x.lo != 0 || x.hi != H) return false;
  return true;
}

int run_plan() {
  Program p;
  // in place over an operand that dies at the step; not when the operand lives on
  p.steps = {level(0)};
  Buffers b = assign_buffers(p);
  CHECK(b.of[1] == 0 && b.count == 1 && b.result == 0);
  p.steps = {rank(0, 3), level(1), table1(2, 3)};
  b = assign_buffers(p);
  CHECK(b.of[1] == 1 && b.of[2] == 1 && b.of[3] == 1);
  p.steps = {level(0), bin(kSubtract, 0, 1)};  // value 0 is read again: the level step may not overwrite it
  b = assign_buffers(p);
  CHECK(b.of[1] != 0 && b.count == 2);
  p.steps = {level(0, 1), level(1, 0)};
  b = assign_buffers(p);
  CHECK(b.of[1] == 0 && b.of[2] == 0 && b.count == 1);
  // nothing folds across a level step; tables on one side of it still do
  p.steps = {table1(0, 1), level(1), table1(2, 2)};
  CHECK(fold(p).size() == 3);
  p.steps = {table1(0, 1), table1(1, 2), level(2), table1(3, 2), table1(4, 0)};
  const Program f = fold(p);
  CHECK(f.size() == 3 && f.steps[0].kind == kTable && f.steps[1].kind == kLevel && f.steps[1].a == 1 &&
        f.steps[2].kind == kTable && f.steps[2].a == 2);
  p.steps = {level(0)};
  CHECK(single_kind(p) == kLevel);
  CHECK(!is_neighbourhood(p.steps[0]) && radius(p.steps[0]) == 0 && reach(p) == 0);
  p.steps = {rank(0, 5), level(1), rank(2, 3)};
  CHECK(reach(p) == 3);
  // whole_frame
  p.steps = {rank(0, 5), table1(1, 1)};
  CHECK(!whole_frame(p));
  p.steps = {rank(0, 5), table1(1, 1), level(2)};
  CHECK(whole_frame(p));
  // rows: whole frames for every value, whatever rows are asked for and wherever the step stands
  const std::vector<std::vector<Step>> progs = {
      {level(0)},
      {rank(0, 5), level(1)},
      {level(0), rank(1, 7)},
      {rank(0, 3), level(1), rank(2, 5), table1(3, 1)},
      {mix(0), level(1, 0, 1), mix(2)},
      {rank(0, 3), level(0, 1), bin(kAbsdiff, 1, 2)},
      {level(0, 1, 0, 0, 655, 655), level(1)},
  };
  for (const std::vector<Step> &steps : progs) {
    p.steps = steps;
    std::string why;
    CHECK(validate(p, 3, &why));
    const Buffers bufs = assign_buffers(p);
    for (int H : {1, 2, 9, 40})
      for (int y0 = 0; y0 < H; y0 += (H > 9 ? 7 : 1))
        for (int y1 : {y0 + 1, H}) {
          CHECK(whole(rows_needed(p, H, y0, y1), H));
          for (const Launch &l : band_launches(p, bufs, H, y0, y1, 0, false))
            CHECK(l.y0 == 0 && l.nrows == H && l.src0 == 0 && l.nsrc == H && l.a_row == 0 && l.dst_row == 0);
        }
    const std::vector<Launch> ls = band_launches(p, bufs, 40, 0, 40, 0, true);
    CHECK(ls.back().dst_buf == kOut && ls.back().dst_row == 0);
  }
  // a program without a level step is cut as before
  p.steps = {rank(0, 5), table1(1, 1)};
  const std::vector<Rows> r = rows_needed(p, 40, 10, 20);
  CHECK(r[2].lo == 10 && r[2].hi == 20 && r[1].lo == 10 && r[1].hi == 20 && r[0].lo == 8 && r[0].hi == 22);
  std::printf("{\"checked\": %d, \"failed\": %d}\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 2 && !std::strcmp(argv[1], "validate")) return run_validate();
  if (argc == 2 && !std::strcmp(argv[1], "plan")) return run_plan();
  std::fprintf(stderr, "usage: chain_plan_level_check validate|plan\n");
  return 2;
}
