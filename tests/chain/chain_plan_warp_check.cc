// chain_plan_warp_check — csrc/vf_chain_plan.h's warp step (kind 12) on the CPU.  Modes:
//   validate   kind 12 is accepted on 1 and 3 channels and its bad arguments are refused with the
//              filter's own words; kinds 11, 13, 4 and -1 stay "unknown kind N"
//   plan       a warp step over a dying operand is NOT placed in place (it reads anywhere in its
//              operand), though it is no neighbourhood step and has radius 0; nothing folds across
//              one; whole_frame; rows_needed and band_launches give whole frames for every value of
//              a program that holds one; the buffer counts of warp -> table, table -> warp ->
//              absdiff with value 0 and two warps in a row; it needs no scratch
// Each prints one JSON line; exit status 1 when a check failed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
Step level(int a) {
  Step s;
  s.kind = kLevel, s.a = a, s.op = vf::level::kEqualize;
  return s;
}
Step warp(int a, int mode = vf::warp::kFlipH, int interp = vf::warp::kNearest, int border = vf::conv::kConstant) {
  Step s;
  s.kind = kWarp, s.a = a, s.border = border;
  const double m[6] = {0.9, 0.1, 2.5, -0.1, 0.9, -1.25};
  std::memcpy(s.warp.m, m, sizeof m);
  s.warp.mode = mode, s.warp.interp = interp;
  s.warp.value[0] = 1, s.warp.value[1] = 2, s.warp.value[2] = 3;
  return s;
}

bool refused(const Program &p, int channels, const char *reason) {
  std::string why;
  return !validate(p, channels, &why) && why.find(reason) != std::string::npos;
}

int run_validate() {
  Program p;
  std::string why;
  CHECK(kWarp == 12 && kClahe == 10 && kLevel == 8 && kSep == 7 && kMix == 5 && kTable == 0 && kConv == 1 && kRank == 2 &&
        kBinary == 3);
  for (int ch : {1, 3})
    for (int mode = 0; mode < 4; ++mode)
      for (int interp = 0; interp < 2; ++interp)
        for (int border = 0; border < 3; ++border) {
          p.steps = {warp(0, mode, interp, border)};
          CHECK(validate(p, ch, &why));
        }
  p.steps = {warp(0, 4)};
  CHECK(refused(p, 3, "step 1: mode=4 outside 0..3"));
  p.steps = {warp(0, 0, 2)};
  CHECK(refused(p, 1, "step 1: interp=2 outside 0..1"));
  p.steps = {warp(0, 0, 0, 3)};
  CHECK(refused(p, 3, "step 1: unknown border 3"));
  p.steps = {table1(0, 1), warp(1, 0)};
  p.steps[1].warp.m[4] = std::numeric_limits<double>::quiet_NaN();
  CHECK(refused(p, 3, "step 2: m[4] is not finite"));
  p.steps[1].warp.mode = vf::warp::kFlipV;  // a flip reads no m
  CHECK(validate(p, 3, &why));
  for (int k : {11, 13, 4, -1}) {  // not kinds
    p.steps = {warp(0)};
    p.steps[0].kind = k;
    CHECK(refused(p, 3, ("step 1: unknown kind " + std::to_string(k)).c_str()));
    CHECK(refused(p, 1, ("step 1: unknown kind " + std::to_string(k)).c_str()));
  }
  p.steps = {warp(1)};  // operands as for every step
  CHECK(refused(p, 3, "operand a = 1 is not an earlier value"));
  p.steps = {warp(0), warp(0)};
  CHECK(refused(p, 3, "value 1 is read by no step"));
  std::printf("{\"checked\": %d, \"failed\": %d}\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}

bool whole(const std::vector<Rows> &r, int H) {
  for (const Rows &x : r)
    if (x.lo != 0 || x.hi != H) return false;
  return true;
}

// No launch of a warp step writes the buffer it reads.
bool warps_out_of_place(const Program &p, const Buffers &bufs, bool to_out) {
  for (const Launch &l : band_launches(p, bufs, 9, 0, 9, 0, to_out))
    if (p.steps[(size_t)l.step - 1].kind == kWarp && l.dst_buf == l.a_buf) return false;
  return true;
}

int run_plan() {
  Program p;
  // never in place, though the operand dies at the step
  p.steps = {warp(0)};
  Buffers b = assign_buffers(p);
  CHECK(b.of[1] == 1 && b.count == 2 && b.result == 1);
  CHECK(scratch_buffers(b, p, true) == 0);  // the result goes to the caller's rows: no scratch buffer
  CHECK(!is_neighbourhood(p.steps[0]) && radius(p.steps[0]) == 0 && reach(p) == 0 && reads_elsewhere(p.steps[0]));
  CHECK(reads_elsewhere(rank(0, 3)) && !reads_elsewhere(table1(0, 1)) && !reads_elsewhere(level(0)) &&
        !reads_elsewhere(bin(kAdd, 0, 0)));
  CHECK(single_kind(p) == kWarp);
  // warp -> table: the table runs in place over the warp's result
  p.steps = {warp(0), table1(1, 3)};
  b = assign_buffers(p);
  CHECK(b.of[1] == 1 && b.of[2] == 1 && b.count == 2 && warps_out_of_place(p, b, false));
  // table -> warp -> absdiff with value 0: the table cannot overwrite value 0, which the absdiff reads
  p.steps = {table1(0, 3), warp(1), bin(kAbsdiff, 0, 2)};
  b = assign_buffers(p);
  CHECK(b.of[0] == 0 && b.of[1] == 1 && b.of[2] == 2 && b.count == 3 && (b.of[3] == 0 || b.of[3] == 2));
  CHECK(warps_out_of_place(p, b, false) && warps_out_of_place(p, b, true));
  // two warps in a row: the second writes the buffer value 0 left
  p.steps = {warp(0), warp(1, vf::warp::kAffine, vf::warp::kLinear)};
  b = assign_buffers(p);
  CHECK(b.of[1] == 1 && b.of[2] == 0 && b.count == 2 && warps_out_of_place(p, b, false));
  p.steps = {warp(0), warp(1), warp(2)};
  b = assign_buffers(p);
  CHECK(b.of[1] == 1 && b.of[2] == 0 && b.of[3] == 1 && b.count == 2 && warps_out_of_place(p, b, false));
  // a warp of a value that is read again
  p.steps = {warp(0), bin(kAbsdiff, 0, 1)};
  b = assign_buffers(p);
  CHECK(b.of[1] == 1 && b.count == 2 && warps_out_of_place(p, b, true));
  // nothing folds across a warp step; tables on one side of it still do
  p.steps = {table1(0, 1), warp(1), table1(2, 2)};
  CHECK(fold(p).size() == 3);
  p.steps = {table1(0, 1), table1(1, 2), warp(2), table1(3, 2), table1(4, 0)};
  const Program f = fold(p);
  CHECK(f.size() == 3 && f.steps[0].kind == kTable && f.steps[1].kind == kWarp && f.steps[1].a == 1 &&
        f.steps[2].kind == kTable && f.steps[2].a == 2);
  p.steps = {rank(0, 5), warp(1), rank(2, 3)};
  CHECK(reach(p) == 3);
  // whole_frame, and no scratch of its own
  p.steps = {rank(0, 5), table1(1, 1)};
  CHECK(!whole_frame(p));
  p.steps = {rank(0, 5), table1(1, 1), warp(2)};
  CHECK(whole_frame(p) && whole_frame_scratch_bytes(p) == level_scratch_bytes());
  // rows: whole frames for every value, whatever rows are asked for and wherever the step stands
  const std::vector<std::vector<Step>> progs = {
      {warp(0)},
      {rank(0, 5), warp(1)},
      {warp(0), rank(1, 7)},
      {rank(0, 3), warp(1), rank(2, 5), table1(3, 1)},
      {table1(0, 3), warp(1), bin(kAbsdiff, 0, 2)},
      {level(0), warp(1, 0, 0, vf::conv::kReflect101)},
      {warp(0), warp(1)},
  };
  for (const std::vector<Step> &steps : progs) {
    p.steps = steps;
    std::string why;
    CHECK(validate(p, 3, &why));
    const Buffers bufs = assign_buffers(p);
    CHECK(warps_out_of_place(p, bufs, false) && warps_out_of_place(p, bufs, true));
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
  // a program without a warp step is cut as before
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
  std::fprintf(stderr, "usage: chain_plan_warp_check validate|plan\n");
  return 2;
}
