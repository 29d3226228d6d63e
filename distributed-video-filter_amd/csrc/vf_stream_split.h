// vf_stream_split.h — how the launchers of the per-byte kernels (vf_stream.h, vf_lut.hip,
// vf_binary.hip, vf_kernels.hip) cut a byte range (host only, no HIP, so
// tests/stream/stream_split_check.cc checks it on the CPU, past any size a test can allocate).
// Not installed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace vf {
namespace stream {

struct Split {
  uint32_t head;  // bytes before the first 16-B boundary (< 16; all of a shorter range)
  uint64_t n16;   // the body: whole 16-B vectors after them
  uint32_t tail;  // bytes after those (< 16)
  uint64_t tail_at() const { return head + (n16 << 4); }  // offset of the tail's first byte
};

// [p, p + nbytes) on the 16-B grid of `aligned_to`, the pointer whose vector accesses the kernel
// keeps aligned: src for invert and lut (dst shares its offset mod 16), dst for shift and binary.
inline Split split(const void *aligned_to, size_t nbytes) {
  const uint32_t head = (uint32_t)((16 - ((uintptr_t)aligned_to & 15)) & 15);
  const uint32_t h = head < nbytes ? head : (uint32_t)nbytes;
  return Split{h, (nbytes - h) >> 4, (uint32_t)((nbytes - h) & 15)};
}

// Bodies above kSplitBytes are cut into equal sub-launches of at most kChunkBytes, issued
// back to back on the stream.  Measured (profiles/r01_large_buffers.txt, tools/tune_invert
// large): ONE grid-stride launch over 1.6-12.7 GB runs at 5.0-5.6 TB/s, the same bytes as
// 192-256 MiB launches at 6.2-6.3 TB/s (64 MiB: 5.7, the grid is then half empty; 1 GiB:
// 6.0).  Each sub-launch is 1.5-2 grid strides, so workgroups re-align at every launch
// boundary instead of drifting apart over tens of strides.
constexpr uint64_t kSplitBytes = 512ull << 20;
constexpr uint64_t kChunkBytes = 256ull << 20;

struct Chunk {
  uint64_t c0, m;    // body vectors [c0, c0 + m)
  bool first, last;  // the launch that also does the head bytes / the tail bytes
};

// The sub-launches of a body of n16 vectors, `tile` vectors per tile: [0, n16) once and in order,
// whole tiles in all but the last.  Always at least one, for the head and tail bytes.
inline std::vector<Chunk> chunks(uint64_t n16, uint64_t tile) {
  const uint64_t nchunks = (n16 << 4) > kSplitBytes ? ((n16 << 4) + kChunkBytes - 1) / kChunkBytes : 1;
  const uint64_t per = nchunks > 1 ? ((n16 + nchunks - 1) / nchunks + tile - 1) / tile * tile : n16;
  std::vector<Chunk> out;
  uint64_t c0 = 0;
  do {
    const uint64_t m = n16 - c0 < per ? n16 - c0 : per;
    out.push_back(Chunk{c0, m, c0 == 0, c0 + m >= n16});
    c0 += m;
  } while (c0 < n16);
  return out;
}

// workgroups of a launch over m body vectors: one per tile, at least one, at most max_blocks
inline unsigned blocks(uint64_t m, uint64_t tile, int max_blocks) {
  const uint64_t tiles = (m + tile - 1) / tile;
  return (unsigned)(tiles == 0 ? 1 : tiles > (uint64_t)max_blocks ? (uint64_t)max_blocks : tiles);
}

// Three interleaved channels, byte i of the range in channel (phase + i) % 3: the channels of the
// first byte of chunk c's body (bits 0-1), of the head (2-3) and of the tail (4-5).
inline uint32_t phases3(uint32_t phase, const Split &s, const Chunk &c) {
  const uint32_t body = (uint32_t)((phase + s.head + (c.c0 << 4)) % 3);
  return body | (phase % 3) << 2 | (uint32_t)((phase + s.tail_at()) % 3) << 4;
}

}  // namespace stream
}  // namespace vf
