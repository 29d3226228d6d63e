// stream_split_check.cc — csrc/vf_stream_split.h on the CPU (built by tests/test_stream_split.py
// with -fsanitize=address,undefined).  Arithmetic only: pointers are numbers, nothing is allocated,
// so the sizes go past what a GPU test can hold.
//
//   stream_split_check TILE
//
// For every pointer offset 0..15 and sizes around 0, 16, a tile of TILE vectors, 512 MiB and
// 12.7 GB (and twice that) it checks that
//   * head + 16 * n16 + tail == nbytes, head < 16, tail < 16, and the body starts on the 16-B grid;
//   * the chunks cover [0, n16) once and in order, every one but the last a whole number of tiles,
//     `first` and `last` each set exactly once; one chunk up to kSplitBytes of body, above that
//     none longer than kChunkBytes;
//   * one launch takes min(max(tiles, 1), max_blocks) workgroups;
//   * for phase 0..2 the three channels phases3 packs are (phase + offset) % 3 at the head (offset
//     0), at each chunk's body and at the tail.
// Prints {"cases", "chunks", "failed"}; exit status 1 when a check failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vf_stream_split.h"

static int g_failed = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (++g_failed <= 20) {                     \
        std::fprintf(stderr, "FAILED %s: ", #cond); \
        std::fprintf(stderr, __VA_ARGS__);        \
        std::fprintf(stderr, "\n");               \
      }                                           \
    }                                             \
  } while (0)

using namespace vf::stream;

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s TILE\n", argv[0]);
    return 2;
  }
  const uint64_t tile = std::strtoull(argv[1], nullptr, 0);
  const uint64_t centres[] = {0, 16, tile * 16, kSplitBytes, 12700000000ull, 25400000000ull};
  const int64_t around[] = {-33, -17, -16, -15, -1, 0, 1, 15, 16, 17, 33};
  std::vector<uint64_t> sizes;
  for (uint64_t c : centres)
    for (int64_t d : around)
      if (d >= 0 || c >= (uint64_t)-d) sizes.push_back(c + (uint64_t)d);
  // around the cut itself: the body, not the range, is what kSplitBytes bounds
  for (uint64_t d = 0; d < 48; ++d) sizes.push_back(kSplitBytes + 16 + d);

  size_t cases = 0, nchunks = 0;
  for (unsigned off = 0; off < 16; ++off) {
    const uintptr_t p = (uintptr_t)0x7f0000001000ull + off;
    for (uint64_t n : sizes) {
      ++cases;
      const Split s = split(reinterpret_cast<const void *>(p), (size_t)n);
      CHECK(s.head + (s.n16 << 4) + s.tail == n, "off %u n %llu: %u + 16 * %llu + %u", off, (unsigned long long)n, s.head,
            (unsigned long long)s.n16, s.tail);
      CHECK(s.head < 16 && s.tail < 16, "off %u n %llu: head %u tail %u", off, (unsigned long long)n, s.head, s.tail);
      CHECK(s.head == n || ((p + s.head) & 15) == 0, "off %u n %llu: the body is off the grid", off, (unsigned long long)n);
      CHECK(s.head == n || s.head == ((16 - off) & 15), "off %u n %llu: head %u", off, (unsigned long long)n, s.head);
      CHECK(s.tail_at() == s.head + s.n16 * 16, "off %u n %llu: tail_at", off, (unsigned long long)n);

      const std::vector<Chunk> cs = chunks(s.n16, tile);
      nchunks += cs.size();
      CHECK(!cs.empty(), "off %u n %llu: no launch for the head and tail", off, (unsigned long long)n);
      const uint64_t body = s.n16 << 4;
      CHECK((cs.size() == 1) == (body <= kSplitBytes), "off %u n %llu: %zu chunks for a body of %llu", off,
            (unsigned long long)n, cs.size(), (unsigned long long)body);
      uint64_t at = 0;
      int firsts = 0, lasts = 0;
      for (size_t k = 0; k < cs.size(); ++k) {
        const Chunk &c = cs[k];
        CHECK(c.c0 == at, "n %llu chunk %zu: starts at %llu, not %llu", (unsigned long long)n, k, (unsigned long long)c.c0,
              (unsigned long long)at);
        CHECK(c.m > 0 || s.n16 == 0, "n %llu chunk %zu: empty", (unsigned long long)n, k);
        CHECK(c.m <= s.n16 - at, "n %llu chunk %zu: past the body", (unsigned long long)n, k);
        if (c.m > s.n16 - at) break;
        if (k + 1 < cs.size()) CHECK(c.m % tile == 0, "n %llu chunk %zu: %llu is no whole number of tiles", (unsigned long long)n, k, (unsigned long long)c.m);
        if (cs.size() > 1) CHECK((c.m << 4) <= kChunkBytes, "n %llu chunk %zu: %llu vectors", (unsigned long long)n, k, (unsigned long long)c.m);
        firsts += c.first;
        lasts += c.last;
        CHECK(c.first == (k == 0) && c.last == (k + 1 == cs.size()), "n %llu chunk %zu: first %d last %d", (unsigned long long)n, k, c.first, c.last);
        const uint64_t tiles = (c.m + tile - 1) / tile;
        for (int mb : {1, 7, 8192}) {
          const uint64_t want = tiles == 0 ? 1 : tiles < (uint64_t)mb ? tiles : (uint64_t)mb;
          CHECK(blocks(c.m, tile, mb) == want, "n %llu chunk %zu max_blocks %d: %u workgroups", (unsigned long long)n, k, mb, blocks(c.m, tile, mb));
        }
        for (uint32_t phase = 0; phase < 3; ++phase) {
          const uint32_t ph = phases3(phase, s, c);
          CHECK(ph < 64, "phases %u", ph);
          CHECK(((ph >> 2) & 3) == phase % 3, "n %llu chunk %zu phase %u: head %u", (unsigned long long)n, k, phase, (ph >> 2) & 3);
          CHECK((ph & 3) == (phase + s.head + 16 * c.c0) % 3, "n %llu chunk %zu phase %u: body %u", (unsigned long long)n, k, phase, ph & 3);
          CHECK(((ph >> 4) & 3) == (phase + s.head + 16 * s.n16) % 3, "n %llu chunk %zu phase %u: tail %u", (unsigned long long)n, k, phase, (ph >> 4) & 3);
        }
        at += c.m;
      }
      CHECK(at == s.n16, "n %llu: chunks end at %llu of %llu", (unsigned long long)n, (unsigned long long)at, (unsigned long long)s.n16);
      CHECK(firsts == 1 && lasts == 1, "n %llu: first set %d times, last %d", (unsigned long long)n, firsts, lasts);
    }
  }
  std::printf("{\"cases\": %zu, \"chunks\": %zu, \"failed\": %d}\n", cases, nchunks, g_failed);
  return g_failed ? 1 : 0;
}
