// pixel_split_check — csrc/vf_pixel_split.h on the CPU: the head / body / tail cut of the
// colour-matrix kernel's launcher, for every offset of dst mod 16 and every length of whole pixels
// up to 300 bytes, plus lengths around 2^32.  Prints one JSON line; exit status 1 when a check failed.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "vf_pixel_split.h"

int main() {
  using vf::pixel::Split;
  using vf::pixel::kUnitBytes;
  long checked = 0, failed = 0, all_head = 0, with_body = 0;
  auto check = [&](uintptr_t dst, uint64_t nbytes) {
    const Split s = vf::pixel::split(reinterpret_cast<const void *>(dst), (size_t)nbytes);
    bool ok = (uint64_t)s.head + s.units * kUnitBytes + s.tail == nbytes;  // they add up
    ok = ok && s.head % 3 == 0 && s.tail % 3 == 0;                         // whole pixels
    ok = ok && s.head < kUnitBytes && s.tail < kUnitBytes;                 // at most 15 pixels each
    ok = ok && s.tail_at() == (uint64_t)s.head + s.units * kUnitBytes;
    if (s.head == nbytes) {  // the range is all head
      ok = ok && s.units == 0 && s.tail == 0;
      ++all_head;
    } else {
      ok = ok && (dst + s.head) % 16 == 0;  // the body starts on dst's 16-B grid ...
      ok = ok && s.head <= 45;              // ... after the SHORTEST such head: 3 k, k < 16
      for (uint32_t h = 0; h < s.head; h += 3) ok = ok && (dst + h) % 16 != 0;
      if (s.units) ++with_body;
    }
    ++checked;
    if (!ok) {
      ++failed;
      fprintf(stderr, "dst %% 16 = %u, nbytes = %llu: head %u units %llu tail %u\n", (unsigned)(dst & 15),
              (unsigned long long)nbytes, s.head, (unsigned long long)s.units, s.tail);
    }
  };
  const uintptr_t base = (uintptr_t)1 << 20;
  for (unsigned off = 0; off < 16; ++off) {
    for (uint64_t n = 0; n <= 300; n += 3) check(base + off, n);
    for (uint64_t n : {((uint64_t)1 << 32) - 1, ((uint64_t)1 << 32) + 2, ((uint64_t)3 << 32) + 48 * 5 + 9})
      check(base + off, n / 3 * 3);
  }
  printf("{\"checked\": %ld, \"failed\": %ld, \"all_head\": %ld, \"with_body\": %ld}\n", checked, failed, all_head,
         with_body);
  return failed ? 1 : 0;
}
