// chain_plan_clahe_check — csrc/vf_chain_plan.h's CLAHE step (kind 10) on the CPU.  Modes:
//   validate   kind 10 is accepted on 1 and 3 channels and its bad arguments are refused with the
//              filter's own words; kinds 4, 6, 9, 11 and -1 stay "unknown kind N"
//   plan       a CLAHE step over a dying operand is placed in place, and not over one that is read
//              again; nothing folds across one; single_kind reports it; whole_frame; its radius and a
//              program's reach do not grow; rows_needed and band_launches give whole frames for
//              every value of a program that holds one, whatever rows are asked for, and bands as
//              before for one that does not; the scratch of a program's level and CLAHE steps
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
Step level(int a) {
  Step s;
  s.kind = kLevel, s.a = a, s.op = vf::level::kEqualize;
  return s;
}
Step clahe(int a, int clip_q8 = 512, int tx = 8, int ty = 8, int mask = 0) {
  Step s;
  s.kind = kClahe, s.a = a, s.clip_q8 = clip_q8, s.tiles_x = tx, s.tiles_y = ty, s.mask = mask;
  return s;
}

bool refused(const Program &p, int channels, const char *reason) {
  std::string why;
  return !validate(p, channels, &why) && why.find(reason) != std::string::npos;
}

int run_validate() {
  Program p;
  std::string why;
  CHECK(kClahe == 10 && kLevel == 8 && kSep == 7 && kMix == 5 && kTable == 0 && kConv == 1 && kRank == 2 && kBinary == 3);
  for (int ch : {1, 3})
    for (int q : {0, 1, 512, 10240, 1 << 24})
      for (int t : {1, 8, 16}) {
        p.steps = {clahe(0, q, t, 17 - t, 0)};
        CHECK(validate(p, ch, &why));
        p.steps = {clahe(0, q, t, t, 1)};
        CHECK(validate(p, ch, &why));
      }
  for (int mask = 0; mask < 8; ++mask) {
    p.steps = {clahe(0, 512, 8, 8, mask)};
    CHECK(validate(p, 3, &why));
  }
  p.steps = {clahe(0, 512, 8, 8, 2)};
  CHECK(refused(p, 1, "step 1: channel mask 2 names a channel beyond the frame's 1"));
  p.steps = {clahe(0, 512, 8, 8, 8)};
  CHECK(refused(p, 3, "step 1: channel mask 8 outside 0..7"));
  p.steps = {clahe(0, -1)};
  CHECK(refused(p, 3, "step 1: clip_q8=-1 outside 0..16777216"));
  p.steps = {clahe(0, (1 << 24) + 1)};
  CHECK(refused(p, 1, "step 1: clip_q8=16777217 outside 0..16777216"));
  p.steps = {clahe(0, 512, 0, 8)};
  CHECK(refused(p, 3, "step 1: tiles_x=0 outside 1..16"));
  p.steps = {clahe(0, 512, 17, 8)};
  CHECK(refused(p, 3, "step 1: tiles_x=17 outside 1..16"));
  p.steps = {clahe(0, 512, 8, 0)};
  CHECK(refused(p, 1, "step 1: tiles_y=0 outside 1..16"));
  p.steps = {clahe(0, 512, 8, 17)};
  CHECK(refused(p, 3, "step 1: tiles_y=17 outside 1..16"));
  p.steps = {table1(0, 1), clahe(1, 512, 8, 8, 4)};
  CHECK(refused(p, 1, "step 2: channel mask 4 names a channel"));
  for (int k : {4, 6, 9, 11, -1}) {  // not kinds
    p.steps = {clahe(0)};
    p.steps[0].kind = k;
    CHECK(refused(p, 3, ("step 1: unknown kind " + std::to_string(k)).c_str()));
    CHECK(refused(p, 1, ("step 1: unknown kind " + std::to_string(k)).c_str()));
  }
  p.steps = {clahe(1)};  // operands as for every step
  CHECK(refused(p, 3, "operand a = 1 is not an earlier value"));
  p.steps = {clahe(0), clahe(0)};
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
  p.steps = {clahe(0)};
  Buffers b = assign_buffers(p);
  CHECK(b.of[1] == 0 && b.count == 1 && b.result == 0);
  p.steps = {rank(0, 3), clahe(1), table1(2, 3)};
  b = assign_buffers(p);
  CHECK(b.of[1] == 1 && b.of[2] == 1 && b.of[3] == 1);
  p.steps = {clahe(0), bin(kSubtract, 0, 1)};  // value 0 is read again: the CLAHE step may not overwrite it
  b = assign_buffers(p);
  CHECK(b.of[1] != 0 && b.count == 2);
  p.steps = {clahe(0, 0, 4, 2), clahe(1)};
  b = assign_buffers(p);
  CHECK(b.of[1] == 0 && b.of[2] == 0 && b.count == 1);
  // nothing folds across a CLAHE step; tables on one side of it still do
  p.steps = {table1(0, 1), clahe(1), table1(2, 2)};
  CHECK(fold(p).size() == 3);
  p.steps = {table1(0, 1), table1(1, 2), clahe(2), table1(3, 2), table1(4, 0)};
  const Program f = fold(p);
  CHECK(f.size() == 3 && f.steps[0].kind == kTable && f.steps[1].kind == kClahe && f.steps[1].a == 1 &&
        f.steps[2].kind == kTable && f.steps[2].a == 2);
  p.steps = {clahe(0)};
  CHECK(single_kind(p) == kClahe);
  CHECK(!is_neighbourhood(p.steps[0]) && radius(p.steps[0]) == 0 && reach(p) == 0);
  p.steps = {rank(0, 5), clahe(1), rank(2, 3)};
  CHECK(reach(p) == 3);
  // whole_frame
  p.steps = {rank(0, 5), table1(1, 1)};
  CHECK(!whole_frame(p));
  p.steps = {rank(0, 5), table1(1, 1), clahe(2)};
  CHECK(whole_frame(p));
  // rows: whole frames for every value, whatever rows are asked for and wherever the step stands
  const std::vector<std::vector<Step>> progs = {
      {clahe(0)},
      {rank(0, 5), clahe(1)},
      {clahe(0), rank(1, 7)},
      {rank(0, 3), clahe(1), rank(2, 5), table1(3, 1)},
      {mix(0), clahe(1, 512, 8, 8, 1), mix(2)},
      {rank(0, 3), clahe(0, 256), bin(kAbsdiff, 1, 2)},
      {level(0), clahe(1, 10240, 16, 1)},
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
  // the scratch: the level steps' words, then a set for every CLAHE step, in the steps' order
  p.steps = {clahe(0), table1(1, 1), level(2), clahe(3, 0, 2, 2)};
  CHECK(level_scratch_bytes() == (size_t)kMaxSteps * vf::level::kHistWords * 4 && level_scratch_bytes() % 16 == 0);
  CHECK(vf::clahe::kScratchBytes % 16 == 0);
  CHECK(whole_frame_scratch_bytes(p) == level_scratch_bytes() + 2 * vf::clahe::kScratchBytes);
  CHECK(clahe_steps_before(p, 1) == 0 && clahe_steps_before(p, 2) == 1 && clahe_steps_before(p, 4) == 1 &&
        clahe_steps_before(p, 5) == 2);
  p.steps = {level(0)};
  CHECK(whole_frame_scratch_bytes(p) == level_scratch_bytes() && whole_frame(p));
  // a program without a CLAHE step is cut as before
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
  std::fprintf(stderr, "usage: chain_plan_clahe_check validate|plan\n");
  return 2;
}
