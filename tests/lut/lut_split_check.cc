// lut_split_check.cc — csrc/vf_lut_split.h on the CPU (built by tests/test_lut_split.py with
// -fsanitize=address,undefined).
//
//   lut_split_check CAPACITY CHANNELS SIZE [SIZE ...]
//
// builds one frame per SIZE inside a source and a destination arena, splits the list and checks
// that the launches tile every frame exactly once and in order, that each fits CAPACITY (and all
// but a frame's last are CAPACITY long), and that each carries phase == offset_in_frame %
// CHANNELS.  Then it runs the launches as the kernel would -- dst[i] = table[(phase + i) %
// CHANNELS][src[i]] -- and compares every frame with the filter applied to the frame as a whole,
// so a wrong phase shows as wrong bytes too.  Prints {"frames", "launches", "failed"}; exit
// status 1 when a check failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vf_lut_split.h"

static int g_failed = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      ++g_failed;                              \
      std::fprintf(stderr, "FAILED %s: ", #cond); \
      std::fprintf(stderr, __VA_ARGS__);       \
      std::fprintf(stderr, "\n");              \
    }                                          \
  } while (0)

int main(int argc, char **argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s CAPACITY CHANNELS SIZE...\n", argv[0]);
    return 2;
  }
  const size_t cap = std::strtoull(argv[1], nullptr, 0);
  const int channels = std::atoi(argv[2]);
  std::vector<size_t> sizes;
  size_t total = 0;
  for (int i = 3; i < argc; ++i) {
    sizes.push_back(std::strtoull(argv[i], nullptr, 0));
    total += sizes.back();
  }
  // exactly `total` bytes each: a launch one byte past a frame is a heap overflow for ASan
  std::vector<uint8_t> src(total), dst(total, 0xEE), want(total);
  std::vector<uint8_t> table((size_t)(channels > 0 ? channels : 1) * 256);
  for (size_t i = 0; i < table.size(); ++i) table[i] = (uint8_t)(i * 167 + 13 + (i >> 8) * 71);
  for (size_t i = 0; i < total; ++i) src[i] = (uint8_t)(i * 131 + 7);
  std::vector<vf::lut::Frame> frames;
  size_t at = 0;
  for (size_t n : sizes) {
    frames.push_back(vf::lut::Frame{src.data() + at, dst.data() + at, n});
    for (size_t i = 0; i < n; ++i) want[at + i] = table[(i % (size_t)(channels > 0 ? channels : 1)) * 256 + src[at + i]];
    at += n;
  }

  const std::vector<vf::lut::Launch> ls = vf::lut::split(frames, cap, channels);
  if (cap == 0 || channels < 1) {
    CHECK(ls.empty(), "capacity 0 or channels < 1 gives no launches, got %zu", ls.size());
    std::printf("{\"frames\": %zu, \"launches\": %zu, \"failed\": %d}\n", frames.size(), ls.size(), g_failed);
    return g_failed ? 1 : 0;
  }
  size_t k = 0;
  for (size_t f = 0; f < frames.size(); ++f) {
    size_t off = 0;
    while (off < frames[f].nbytes) {
      CHECK(k < ls.size(), "frame %zu: launches end at offset %zu of %zu", f, off, frames[f].nbytes);
      if (k >= ls.size()) break;
      const vf::lut::Launch &l = ls[k];
      CHECK(l.src == frames[f].src + off && l.dst == frames[f].dst + off, "frame %zu launch %zu: not at offset %zu", f, k, off);
      CHECK(l.len >= 1 && l.len <= cap, "launch %zu: len %zu outside 1..%zu", k, l.len, cap);
      CHECK(l.len <= frames[f].nbytes - off, "launch %zu: %zu bytes past its frame's %zu left", k, l.len, frames[f].nbytes - off);
      CHECK(l.len == cap || off + l.len == frames[f].nbytes, "launch %zu: short (%zu) before its frame's end", k, l.len);
      CHECK(l.phase == (uint32_t)(off % (size_t)channels), "launch %zu: phase %u at offset %zu", k, l.phase, off);
      if (l.len == 0 || l.len > frames[f].nbytes - off) break;
      off += l.len;
      ++k;
    }
  }
  CHECK(k == ls.size(), "%zu launches beyond the frames", ls.size() - k);
  if (!g_failed) {
    for (const vf::lut::Launch &l : ls)
      for (size_t i = 0; i < l.len; ++i) l.dst[i] = table[((l.phase + i) % (size_t)channels) * 256 + l.src[i]];
    size_t bad = 0;
    for (size_t i = 0; i < total; ++i) bad += dst[i] != want[i];
    CHECK(bad == 0, "%zu of %zu bytes differ from the whole-frame filter", bad, total);
  }
  std::printf("{\"frames\": %zu, \"launches\": %zu, \"failed\": %d}\n", frames.size(), ls.size(), g_failed);
  return g_failed ? 1 : 0;
}
