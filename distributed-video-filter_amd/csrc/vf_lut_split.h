// vf_lut_split.h — how a list of frames is cut into LUT kernel launches (host only, no HIP, so
// tests/lut/lut_split_check.cc checks it on the CPU).  Not installed.
//
// A frame of an interleaved 3-channel image starts at channel 0 and byte i of it goes through
// table i % 3.  A frame larger than the staging capacity is cut wherever the capacity ends, not
// at a pixel boundary, so every launch carries the channel of its first byte (`phase`); the
// kernel (vf_lut.hip) counts on from there.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace vf {
namespace lut {

struct Frame {
  const uint8_t *src;
  uint8_t *dst;
  size_t nbytes;
};

struct Launch {
  const uint8_t *src;
  uint8_t *dst;
  size_t len;      // 1 .. capacity
  uint32_t phase;  // channel of src[0]: its offset in the frame mod channels
};

// The launches of `frames` in order: each frame's bytes exactly once, front to back, in pieces
// of at most `capacity` bytes (all but a frame's last piece are `capacity` long); empty frames
// give none.  capacity == 0 or channels < 1 gives no launches at all.
inline std::vector<Launch> split(const std::vector<Frame> &frames, size_t capacity, int channels) {
  std::vector<Launch> out;
  if (capacity == 0 || channels < 1) return out;
  for (const Frame &f : frames) {
    for (size_t off = 0; off < f.nbytes;) {
      const size_t left = f.nbytes - off;
      const size_t len = left < capacity ? left : capacity;
      out.push_back(Launch{f.src + off, f.dst + off, len, (uint32_t)(off % (size_t)channels)});
      off += len;
    }
  }
  return out;
}

}  // namespace lut
}  // namespace vf
