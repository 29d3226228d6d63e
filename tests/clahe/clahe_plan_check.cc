// clahe_plan_check — csrc/vf_clahe_plan.h on the CPU.  Modes:
//   limits    every refusal of the filter's arguments and of a frame's size, with its message
//   geometry  reads lines "W H tiles_x tiles_y" and prints "We He tw th area" and then the source
//             index of every extended column and row that lies past the frame
//   clip      reads lines "clip_q8 area" and prints clip_of
//   table     reads lines "area clip h[0] .. h[255]" (clip in counts, 0: none) and prints clahe_table's
//             256 entries, one line of integers per histogram
//   weights   reads lines "n side tiles" and prints for every x of 0 .. n - 1 "t1 t2 raw a a1", the
//             floats as their bit patterns, then the axis' cell starts for k = -1 .. tiles
//   pixel     reads lines "t11 t12 t21 t22 xa xa1 ya ya1" (the floats as bit patterns) and prints clahe_pixel
// limits prints one JSON line; exit status 1 when a check failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "vf_clahe_plan.h"

using namespace vf::clahe;

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

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

bool refused(int clip_q8, int tx, int ty, int mask, int channels, const char *reason) {
  std::string why;
  return !limits_ok(clip_q8, tx, ty, mask, channels, &why) && why.find(reason) != std::string::npos;
}

int run_limits() {
  std::string why;
  CHECK(kMaxTilesAxis == 16 && kMaxTiles == 256 && kMaxClipQ8 == 1 << 24 && kStepData == 4);
  CHECK(kScratchBytes == 960 * 1024 && kHistWords == 196608 && kTableBytes == 196608);
  CHECK(hist_words(8, 8, 3) == 49152 && table_bytes(16, 16, 1) == 65536);
  for (int ch : {1, 3})
    for (int q : {0, 1, 256, 512, 640, 10240, 1 << 24})
      for (int t : {1, 8, 16}) CHECK(limits_ok(q, t, 17 - t, 0, ch, &why) && limits_ok(q, t, t, 1, ch, &why));
  for (int mask = 0; mask < 8; ++mask) CHECK(limits_ok(512, 8, 8, mask, 3, &why));
  for (int mask : {2, 3, 4, 5, 6, 7}) CHECK(refused(512, 8, 8, mask, 1, "names a channel beyond the frame's 1"));
  CHECK(refused(512, 8, 8, 8, 3, "channel mask 8 outside 0..7"));
  CHECK(refused(512, 8, 8, -1, 3, "channel mask -1 outside 0..7"));
  CHECK(refused(-1, 8, 8, 0, 3, "clip_q8=-1 outside 0..16777216"));
  CHECK(refused((1 << 24) + 1, 8, 8, 0, 1, "clip_q8=16777217 outside 0..16777216"));
  CHECK(refused(512, 0, 8, 0, 3, "tiles_x=0 outside 1..16"));
  CHECK(refused(512, 17, 8, 0, 3, "tiles_x=17 outside 1..16"));
  CHECK(refused(512, 8, 0, 0, 3, "tiles_y=0 outside 1..16"));
  CHECK(refused(512, 8, 17, 0, 1, "tiles_y=17 outside 1..16"));
  CHECK(refused(512, 8, -3, 0, 1, "tiles_y=-3 outside 1..16"));
  CHECK(refused(512, 8, 8, 0, 2, "channels=2, a frame has 1 or 3"));
  CHECK(refused(512, 8, 8, 0, 4, "channels=4, a frame has 1 or 3"));
  // a frame's size
  CHECK(frame_ok(1920, 1080, 8, 8, &why) && frame_ok(1, 1, 16, 16, &why) && frame_ok(65535, 65535, 2, 2, &why));
  CHECK(!frame_ok(1ull << 20, 1ull << 20, 8, 8, &why) && why.find("a frame of 1099511627776 pixels; at most 4294967295") == 0);
  CHECK(!frame_ok((1ull << 30) + 1, 1, 8, 8, &why) && why.find("a side is at most 1073741824") != std::string::npos);
  CHECK(!frame_ok(65535, 65535, 1, 1, &why) && why.find("a tile of 65535 x 65535 pixels; its area must be at most 2147483647") == 0);
  CHECK(frame_ok(46340, 46340, 1, 1, &why) && !frame_ok(46341, 46341, 1, 1, &why));
  CHECK(resolved_mask(0, 1) == 1 && resolved_mask(0, 3) == 7 && resolved_mask(2, 3) == 2);
  std::printf("{\"checked\": %d, \"failed\": %d}\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}

int bad_line(const char *what) {
  std::fprintf(stderr, "a line does not hold %s\n", what);
  return 2;
}

int run_geometry() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    uint32_t W, H;
    int tx, ty;
    in >> W >> H >> tx >> ty;
    if (!in) return bad_line("W H tiles_x tiles_y");
    const Geometry g = geometry(W, H, tx, ty);
    std::printf("%u %u %u %u %llu", g.We, g.He, g.tw, g.th, (unsigned long long)g.area);
    for (uint32_t p = W; p < g.We; ++p) std::printf(" %u", source_index(p, W));
    for (uint32_t p = H; p < g.He; ++p) std::printf(" %u", source_index(p, H));
    std::printf("\n");
  }
  return 0;
}

int run_clip() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    int q;
    unsigned long long area;
    in >> q >> area;
    if (!in) return bad_line("clip_q8 area");
    std::printf("%llu\n", (unsigned long long)clip_of(q, area));
  }
  return 0;
}

int run_table() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    unsigned long long area, clip;
    uint32_t h[256];
    in >> area >> clip;
    for (int v = 0; v < 256; ++v) in >> h[v];
    if (!in) return bad_line("the area, the clip and 256 bins");
    uint8_t out[256];
    clahe_table(h, area, clip, out);
    for (int v = 0; v < 256; ++v) std::printf("%d%c", (int)out[v], v == 255 ? '\n' : ' ');
  }
  return 0;
}

int run_weights() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    uint32_t n, side;
    int tiles;
    in >> n >> side >> tiles;
    if (!in) return bad_line("n side tiles");
    const float inv = clahe_inv(side);
    for (uint32_t x = 0; x < n; ++x) {
      const Weights w = clahe_weights(x, inv, tiles);
      std::printf("%d %d %d %u %u ", w.t1, w.t2, w.raw, bits(w.a), bits(w.a1));
    }
    for (int k = -1; k <= tiles; ++k) std::printf("%u ", cell_start(k, side, inv, tiles, n));
    std::printf("\n");
  }
  return 0;
}

int run_pixel() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    uint32_t t[4], f[4];
    for (uint32_t &v : t) in >> v;
    for (uint32_t &v : f) in >> v;
    if (!in) return bad_line("four entries and four weights");
    std::printf("%u\n", clahe_pixel(t[0], t[1], t[2], t[3], from_bits(f[0]), from_bits(f[1]), from_bits(f[2]), from_bits(f[3])));
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 2 && !std::strcmp(argv[1], "limits")) return run_limits();
  if (argc == 2 && !std::strcmp(argv[1], "geometry")) return run_geometry();
  if (argc == 2 && !std::strcmp(argv[1], "clip")) return run_clip();
  if (argc == 2 && !std::strcmp(argv[1], "table")) return run_table();
  if (argc == 2 && !std::strcmp(argv[1], "weights")) return run_weights();
  if (argc == 2 && !std::strcmp(argv[1], "pixel")) return run_pixel();
  std::fprintf(stderr, "usage: clahe_plan_check limits|geometry|clip|table|weights|pixel\n");
  return 2;
}
