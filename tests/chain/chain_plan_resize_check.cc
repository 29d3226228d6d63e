// chain_plan_resize_check — csrc/vf_chain_plan.h's resize step (kind 14) on the CPU.  Modes:
//   validate   kind 14 is accepted on 1 and 3 channels and its bad arguments are refused with the
//              filter's own words; kinds 13, 15, 4 and -1 stay "unknown kind N"
//   plan       value_sizes through shrink -> median -> upscale; a binary step on values of unequal
//              size is refused, naming the step; a resize step over a dying operand is NOT placed in
//              place; nothing folds across one; whole_frame; frame_launches carries the sizes;
//              buffer_bytes gives the largest value a buffer holds; assign_buffers' keep_input keeps
//              buffer 0 for the frame alone; for programs without a resize
//              step frame_launches equals band_launches of the whole frame
//   launches   the launches of a few programs WITHOUT a resize step, whole frames and bands, one line
//              a launch list: tests/golden/chain_plan_launches.json holds what the header gave before
//              it knew sizes, and this mode compiles against that header as well (-DLAUNCHES_ONLY)
// validate and plan print one JSON line; exit status 1 when a check failed.
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
Step level(int a) {
  Step s;
  s.kind = kLevel, s.a = a, s.op = vf::level::kEqualize;
  return s;
}

// The programs of the launches mode: none holds a resize step.
std::vector<Program> old_programs() {
  std::vector<Program> ps(5);
  ps[0].steps = {rank(0, 3)};
  ps[1].steps = {rank(0, 3), rank(1, 5), bin(kSubtract, 1, 2)};
  ps[2].steps = {table1(0, 0), rank(1, 7), table1(2, 3), bin(kAbsdiff, 0, 3)};
  ps[3].steps = {rank(0, 3), level(1), table1(2, 5)};
  ps[4].steps = {table1(0, 1), bin(kMax, 0, 1), rank(2, 5), rank(3, 3), bin(kMin, 2, 4)};
  return ps;
}

void print_launches(const std::vector<Launch> &ls) {
  for (const Launch &l : ls)
    std::printf("%d %d %d %d %d %d %d %d %d %d %d  ", l.step, l.a_buf, l.b_buf, l.dst_buf, l.a_row, l.b_row, l.dst_row, l.y0, l.nrows,
                l.src0, l.nsrc);
  std::printf("\n");
}

int run_launches() {
  for (const Program &in : old_programs()) {
    const Program p = fold(in);
    const Buffers b = assign_buffers(p);
    for (int to_out = 0; to_out < 2; ++to_out) {
      print_launches(band_launches(p, b, 40, 0, 40, 0, to_out != 0));
      if (!whole_frame(p)) {
        print_launches(band_launches(p, b, 40, 10, 25, 10 - std::min(10, reach(p)), to_out != 0));
        print_launches(band_launches(p, b, 40, 30, 40, 30 - reach(p), to_out != 0));
      }
    }
  }
  return 0;
}

#ifndef LAUNCHES_ONLY

Step resize(int a, int dw, int dh, double fx = 0, double fy = 0, int interp = vf::resize::kLinear) {
  Step s;
  s.kind = kResize, s.a = a;
  s.resize.dw = dw, s.resize.dh = dh, s.resize.fx = fx, s.resize.fy = fy, s.resize.interp = interp;
  return s;
}

bool refused(const Program &p, int channels, const char *reason) {
  std::string why;
  return !validate(p, channels, &why) && why.find(reason) != std::string::npos;
}

int run_validate() {
  Program p;
  std::string why;
  CHECK(kResize == 14 && kWarp == 12 && kClahe == 10 && kLevel == 8 && kSep == 7 && kMix == 5 && kTable == 0 && kConv == 1 &&
        kRank == 2 && kBinary == 3);
  for (int ch : {1, 3})
    for (int interp : {0, 1, 3}) {
      p.steps = {resize(0, 10, 7, 0, 0, interp)};
      CHECK(validate(p, ch, &why));
      p.steps = {resize(0, 0, 0, 0.5, 1.5, interp)};
      CHECK(validate(p, ch, &why));
    }
  p.steps = {resize(0, 10, 7, 0, 0, 2)};
  CHECK(refused(p, 3, "step 1: interpolation 2 (cubic, Lanczos) is not built"));
  p.steps = {resize(0, 10, 7, 0, 0, 4)};
  CHECK(refused(p, 3, "step 1: interpolation 4"));
  p.steps = {resize(0, 10, 7, 0, 0, 5)};
  CHECK(refused(p, 3, "step 1: unknown interpolation 5"));
  p.steps = {resize(0, 32768, 7)};
  CHECK(refused(p, 3, "step 1: dsize 32768 x 7; a side is 1 to 32767"));
  p.steps = {resize(0, 10, 0)};
  CHECK(refused(p, 3, "step 1: dsize 10 x 0 has a side of 0"));
  p.steps = {resize(0, 0, 0, 0.0, 1.0)};
  CHECK(refused(p, 3, "step 1: without dsize, fx and fy are finite and positive"));
  p.steps = {table1(0, 0), resize(1, 10, 7, 0, 0, -1)};
  CHECK(refused(p, 1, "step 2: unknown interpolation -1"));
  for (int kind : {13, 15, 4, -1, 11, 16}) {
    Step s;
    s.kind = kind, s.a = 0;
    p.steps = {s};
    CHECK(refused(p, 3, ("step 1: unknown kind " + std::to_string(kind)).c_str()));
  }
  p.steps = {resize(1, 10, 7)};
  CHECK(refused(p, 3, "operand a = 1 is not an earlier value"));
  p.steps = {resize(0, 10, 7), resize(0, 5, 5)};
  CHECK(refused(p, 3, "value 1 is read by no step"));
  std::printf("{\"checked\": %d, \"failed\": %d}\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}

bool same_size(const Size &s, int w, int h) { return s.w == w && s.h == h; }

int run_plan() {
  std::string why;
  std::vector<Size> z;
  // shrink -> median -> upscale: 100 x 60 -> 50 x 30 -> 50 x 30 -> 100 x 60
  Program p;
  p.steps = {resize(0, 0, 0, 0.5, 0.5), rank(1, 3), resize(2, 100, 60)};
  CHECK(validate(p, 3, &why) && has_resize(p) && whole_frame(p) && reach(p) == 1);
  CHECK(value_sizes(p, 100, 60, &z, &why) && z.size() == 4);
  CHECK(same_size(z[0], 100, 60) && same_size(z[1], 50, 30) && same_size(z[2], 50, 30) && same_size(z[3], 100, 60));
  CHECK(value_sizes(p, 5, 7, &z, &why) && same_size(z[1], 2, 4) && same_size(z[3], 100, 60));  // half to even
  CHECK(!value_sizes(p, 1, 1, &z, &why) && why.find("step 1: a frame of 1 x 1 resizes to 0 x 0: a side of 0") != std::string::npos);
  {
    const Program f = fold(p);
    CHECK(f.size() == 3);
    const Buffers b = assign_buffers(f);
    // none of the three writes the buffer it reads: the resizes are not in place, nor is the median
    CHECK(b.of[1] != b.of[0] && b.of[2] != b.of[1] && b.of[3] != b.of[2]);
    value_sizes(f, 100, 60, &z, &why);
    const std::vector<Launch> ls = frame_launches(f, b, z, true);
    CHECK(ls.size() == 3);
    CHECK(ls[0].a_w == 100 && ls[0].a_h == 60 && ls[0].w == 50 && ls[0].h == 30 && ls[0].nrows == 30 && ls[0].nsrc == 30);
    CHECK(ls[1].a_w == 50 && ls[1].a_h == 30 && ls[1].w == 50 && ls[1].h == 30 && ls[1].nrows == 30 && ls[1].nsrc == 30 &&
          ls[1].src0 == 0 && ls[1].y0 == 0);
    CHECK(ls[2].a_w == 50 && ls[2].a_h == 30 && ls[2].w == 100 && ls[2].h == 60 && ls[2].nrows == 60 && ls[2].dst_buf == kOut);
    for (const Launch &l : ls) CHECK(l.a_row == 0 && l.b_row == 0 && l.dst_row == 0 && (l.dst_buf == kOut || l.dst_buf != l.a_buf));
    const std::vector<size_t> bytes = buffer_bytes(b, z, 3);
    CHECK((int)bytes.size() == b.count);
    for (int k = 0; k < b.count; ++k) {  // the largest value the buffer holds
      size_t want = 0;
      for (int v = 0; v <= 3; ++v)
        if (b.of[v] == k) want = std::max(want, (size_t)z[v].w * z[v].h * 3);
      CHECK(bytes[(size_t)k] == want);
    }
    CHECK(bytes[0] >= (size_t)100 * 60 * 3);
  }
  // a resize step over a dying operand, between tables: never in place, nothing folds across it
  p.steps = {table1(0, 0), resize(1, 20, 10), table1(2, 3)};
  CHECK(validate(p, 1, &why));
  {
    const Program f = fold(p);
    CHECK(f.size() == 3 && f.steps[1].kind == kResize);
    const Buffers b = assign_buffers(f);
    CHECK(b.of[1] == b.of[0]);  // the table runs in place over the dying frame ...
    CHECK(b.of[2] != b.of[1]);  // ... the resize does not ...
    CHECK(b.of[3] == b.of[2]);  // ... and the table behind it does again
    CHECK(value_sizes(f, 64, 48, &z, &why));
    const std::vector<size_t> bytes = buffer_bytes(b, z, 1);
    CHECK(bytes[(size_t)b.of[0]] == 64 * 48 && bytes[(size_t)b.of[2]] == 20 * 10);
  }
  // keep_input (the JPEG path under a resize step): buffer 0 holds value 0 and nothing else, ever
  for (const Program &in : {p, Program{{resize(0, 0, 0, 0.5, 0.5), rank(1, 3), resize(2, 100, 60)}},
                            Program{{table1(0, 1), bin(kMax, 0, 1), resize(2, 9, 9), table1(3, 2)}}}) {
    const Program f = fold(in);
    const Buffers b = assign_buffers(f, true), plain = assign_buffers(f);
    CHECK(b.of[0] == 0 && b.result != 0);
    for (int v = 1; v <= f.size(); ++v) CHECK(b.of[v] != 0);
    for (int i = 1; i <= f.size(); ++i)  // and a step that reads elsewhere still never writes what it reads
      if (reads_elsewhere(f.steps[i - 1])) CHECK(b.of[i] != b.of[f.steps[i - 1].a]);
    CHECK(b.count >= plain.count);
  }
  // two values resized to one size meet in a binary step; unequal sizes are refused, naming the step
  p.steps = {resize(0, 40, 30), resize(0, 40, 30, 0, 0, vf::resize::kNearest), bin(kAbsdiff, 1, 2)};
  CHECK(validate(p, 3, &why) && value_sizes(p, 160, 48, &z, &why) && same_size(z[3], 40, 30));
  p.steps = {resize(0, 0, 0, 0.5, 0.5), bin(kAbsdiff, 0, 1)};
  CHECK(validate(p, 3, &why));
  CHECK(!value_sizes(p, 160, 48, &z, &why));
  CHECK(why.find("step 2: operand a (value 0) is 160 x 48 and operand b (value 1) is 80 x 24") != std::string::npos);
  p.steps = {resize(0, 40, 30), resize(1, 30, 10, 0, 0, vf::resize::kArea)};  // area at 4 / 3
  CHECK(validate(p, 3, &why) && !value_sizes(p, 160, 48, &z, &why) && why.find("step 2: area from 40 x 30 to 30 x 10") != std::string::npos);
  // without a resize step every value has the frame's size, and frame_launches is band_launches of the whole frame
  for (const Program &in : old_programs()) {
    const Program f = fold(in);
    CHECK(!has_resize(f));
    const Buffers b = assign_buffers(f);
    CHECK(value_sizes(f, 33, 40, &z, &why));
    for (const Size &s : z) CHECK(same_size(s, 33, 40));
    for (int to_out = 0; to_out < 2; ++to_out) {
      const std::vector<Launch> a = frame_launches(f, b, z, to_out != 0), w = band_launches(f, b, 40, 0, 40, 0, to_out != 0);
      CHECK(a.size() == w.size());
      for (size_t i = 0; i < a.size() && i < w.size(); ++i) {
        CHECK(a[i].step == w[i].step && a[i].a_buf == w[i].a_buf && a[i].b_buf == w[i].b_buf && a[i].dst_buf == w[i].dst_buf &&
              a[i].a_row == w[i].a_row && a[i].b_row == w[i].b_row && a[i].dst_row == w[i].dst_row && a[i].y0 == w[i].y0 &&
              a[i].nrows == w[i].nrows && a[i].src0 == w[i].src0 && a[i].nsrc == w[i].nsrc);
        CHECK(w[i].a_w == 0 && w[i].w == 0 && a[i].a_w == 33 && a[i].h == 40);
      }
    }
  }
  std::printf("{\"checked\": %d, \"failed\": %d}\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}

#endif  // LAUNCHES_ONLY

}  // namespace

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "launches") return run_launches();
#ifndef LAUNCHES_ONLY
  if (mode == "validate") return run_validate();
  if (mode == "plan") return run_plan();
#endif
  std::fprintf(stderr, "usage: chain_plan_resize_check validate|plan|launches\n");
  return 2;
}
