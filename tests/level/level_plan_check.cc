// level_plan_check — csrc/vf_level_plan.h on the CPU.  Modes:
//   limits   every refusal of the filter's arguments and of a frame's size, with its message
//   table    reads lines "rule clip_lo clip_hi total h[0] .. h[255]" from stdin and prints
//            level_table's 256 entries for each, one line of integers per histogram
// limits prints one JSON line; exit status 1 when a check failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "vf_level_plan.h"

using namespace vf::level;

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

bool refused(int rule, int mask, int link, int lo, int hi, int channels, const char *reason) {
  std::string why;
  return !limits_ok(rule, mask, link, lo, hi, channels, &why) && why.find(reason) != std::string::npos;
}

int run_limits() {
  std::string why;
  CHECK(kEqualize == 0 && kStretch == 1 && kMaxClip == 32767 && kStepData == 4 && kHistWords == 768);
  for (int ch : {1, 3})
    for (int link : {0, 1}) {
      CHECK(limits_ok(kEqualize, 0, link, 0, 0, ch, &why));
      CHECK(limits_ok(kStretch, 0, link, 0, 0, ch, &why));
      CHECK(limits_ok(kStretch, 1, link, 32767, 32767, ch, &why));
      CHECK(limits_ok(kStretch, 1, link, 0, 655, ch, &why));
    }
  for (int mask = 0; mask < 8; ++mask) CHECK(limits_ok(kEqualize, mask, 0, 0, 0, 3, &why));
  CHECK(limits_ok(kEqualize, 1, 0, 0, 0, 1, &why));
  for (int mask : {2, 3, 4, 5, 6, 7}) CHECK(refused(kEqualize, mask, 0, 0, 0, 1, "names a channel beyond the frame's 1"));
  CHECK(refused(kEqualize, 8, 0, 0, 0, 3, "channel mask 8 outside 0..7"));
  CHECK(refused(kEqualize, -1, 0, 0, 0, 3, "channel mask -1 outside 0..7"));
  CHECK(refused(2, 0, 0, 0, 0, 3, "unknown level rule 2"));
  CHECK(refused(-1, 0, 0, 0, 0, 1, "unknown level rule -1"));
  CHECK(refused(kEqualize, 0, 0, 0, 0, 2, "channels=2, a frame has 1 or 3"));
  CHECK(refused(kEqualize, 0, 0, 0, 0, 4, "channels=4, a frame has 1 or 3"));
  CHECK(refused(kEqualize, 0, 2, 0, 0, 3, "link=2 is not 0 or 1"));
  CHECK(refused(kStretch, 0, -1, 0, 0, 3, "link=-1 is not 0 or 1"));
  CHECK(refused(kStretch, 0, 0, 32768, 0, 3, "clips 32768, 0 outside 0..32767"));
  CHECK(refused(kStretch, 0, 0, 0, 32768, 3, "clips 0, 32768 outside 0..32767"));
  CHECK(refused(kStretch, 0, 0, -1, 0, 1, "clips -1, 0 outside 0..32767"));
  CHECK(refused(kEqualize, 0, 0, 1, 0, 3, "the equalize rule takes no clips"));
  CHECK(refused(kEqualize, 0, 0, 0, 1, 1, "the equalize rule takes no clips"));
  // a frame's size
  CHECK(pixels_ok(0xFFFFFFFFull, 0, 0, 3, &why));
  CHECK(pixels_ok(0xFFFFFFFFull, 1, 1, 3, &why));  // one linked channel sums nothing
  CHECK(!pixels_ok(0x100000000ull, 0, 0, 1, &why) && why.find("a frame of 4294967296 pixels; at most 4294967295") == 0);
  CHECK(!pixels_ok(0x80000000ull, 0, 1, 3, &why) && why.find("linked channels of 2147483648 pixels sum to 6442450944") == 0);
  CHECK(!pixels_ok(0x80000000ull, 5, 1, 3, &why) && why.find("sum to 4294967296 entries") != std::string::npos);
  CHECK(pixels_ok(0x7FFFFFFFull, 5, 1, 3, &why));
  CHECK(pixels_ok(0x55555555ull, 0, 1, 3, &why) && !pixels_ok(0x55555556ull, 7, 1, 3, &why));
  CHECK(mask_count(0) == 0 && mask_count(5) == 2 && mask_count(7) == 3 && resolved_mask(0, 1) == 1 &&
        resolved_mask(0, 3) == 7 && resolved_mask(2, 3) == 2);
  CHECK(cut(0xFFFFFFFFull, 32767) == ((0xFFFFFFFFull * 32767) >> 16) && cut(100, 655) == 0 && cut(101, 655) == 1);
  std::printf("{\"checked\": %d, \"failed\": %d}\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}

int run_table() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    int rule, clip_lo, clip_hi;
    unsigned long long total;
    uint32_t h[256];
    in >> rule >> clip_lo >> clip_hi >> total;
    for (int v = 0; v < 256; ++v) in >> h[v];
    if (!in) {
      std::fprintf(stderr, "a line does not hold rule, two clips, the total and 256 bins\n");
      return 2;
    }
    uint8_t out[256];
    level_table(h, total, rule, clip_lo, clip_hi, out);
    for (int v = 0; v < 256; ++v) std::printf("%d%c", (int)out[v], v == 255 ? '\n' : ' ');
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 2 && !std::strcmp(argv[1], "limits")) return run_limits();
  if (argc == 2 && !std::strcmp(argv[1], "table")) return run_table();
  std::fprintf(stderr, "usage: level_plan_check limits|table\n");
  return 2;
}
