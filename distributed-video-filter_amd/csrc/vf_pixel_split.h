// vf_pixel_split.h — how the launcher of the colour-matrix kernel (vf_mix.hip) cuts a range of
// whole 3-byte pixels (host only, no HIP, so tests/mix/pixel_split_check.cc checks it on the
// CPU).  Not installed.
//
// The kernel's lane works on a unit of 48 B: 16 pixels, three 16-B vectors.  Its body must start
// where a pixel starts AND where dst is 16-B aligned, so the head is h bytes with h % 3 == 0 and
// (dst + h) % 16 == 0.  3 is invertible mod 16 (3 * 11 = 33 = 1), so h = 3 k with
// k = 11 * (-dst mod 16) mod 16 always exists and 0 <= h <= 45: at most 15 pixels.  What is left
// after the whole units is the tail: under 48 B, whole pixels again.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vf {
namespace pixel {

constexpr uint32_t kUnitBytes = 48;  // 16 pixels of 3 bytes = 3 vectors of 16 B

struct Split {
  uint32_t head;   // bytes before the body: a multiple of 3, < 48 (all of a shorter range)
  uint64_t units;  // the body: whole 48-B units after them, the first at a 16-B boundary of dst
  uint32_t tail;   // bytes after those: a multiple of 3, < 48
  uint64_t tail_at() const { return head + units * kUnitBytes; }  // offset of the tail's first byte
};

// [dst, dst + nbytes), nbytes % 3 == 0, on dst's 16-B grid and the pixel grid at once.
inline Split split(const void *dst, size_t nbytes) {
  const uint32_t to16 = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
  const uint32_t head = 3 * ((to16 * 11) & 15);  // head % 16 == to16
  if (head >= nbytes) return Split{(uint32_t)nbytes, 0, 0};
  const size_t rest = nbytes - head;
  return Split{head, rest / kUnitBytes, (uint32_t)(rest % kUnitBytes)};
}

}  // namespace pixel
}  // namespace vf
