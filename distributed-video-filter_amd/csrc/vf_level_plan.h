// vf_level_plan.h — what the level filter (vf_level.hip; cv2.equalizeHist, auto-levels; DESIGN.md
// 22) decides outside its streaming loops: the limits of its arguments, the layout of a
// VF_STEP_LEVEL step's data, and THE TABLE RULE, from a 256-bin histogram to a 256-entry table.
// The rule's text compiles for the host (no HIP include is needed: tests/level/level_plan_check.cc
// checks it on the CPU) and for the device, where the kernel calls the same level_scalars' searches
// over a parallel scan and the same level_entry per bin.  Not installed.
#pragma once
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
// correctly rounded whatever the compiler flags say about fast math
#define VF_LEVEL_FN __host__ __device__ inline
#define VF_LEVEL_U2F(x) __uint2float_rn(x)
#define VF_LEVEL_FDIV(a, b) __fdiv_rn((a), (b))
#define VF_LEVEL_FMUL(a, b) __fmul_rn((a), (b))
#define VF_LEVEL_F2I(x) __float2int_rn(x)
#else
#include <cmath>
#if defined(__HIPCC__)
#define VF_LEVEL_FN __host__ __device__ inline
#else
#define VF_LEVEL_FN inline
#endif
// IEEE single precision on the host: the conversion rounds to nearest even, the divide and the
// multiply are single operations (no fused form exists for either alone), nearbyint rounds half
// to even in the default rounding mode.
#define VF_LEVEL_U2F(x) ((float)(uint32_t)(x))
#define VF_LEVEL_FDIV(a, b) ((float)(a) / (float)(b))
#define VF_LEVEL_FMUL(a, b) ((float)(a) * (float)(b))
#define VF_LEVEL_F2I(x) ((int)std::nearbyint(x))
#endif

#include <string>

namespace vf {
namespace level {

constexpr int kEqualize = 0, kStretch = 1;  // VF_LEVEL_*
constexpr int kMaxClip = 32767;             // clip_lo, clip_hi: units of 1 / 65536 of the total
constexpr uint64_t kMaxPixels = 0xFFFFFFFFull;  // of a frame: every count fits 32 bits
constexpr int kStepData = 4;                // a VF_STEP_LEVEL step's data: {mask, link, clip_lo, clip_hi} as int32
constexpr int kHistWords = 3 * 256;         // the histogram words of one level step (a 1-channel frame uses 256)

// What the rule reads of a histogram besides one bin's running sum.
struct Scalars {
  uint32_t lo, hi;  // equalize: lo = i0; stretch: the clipped range's ends
  uint32_t base;    // equalize: h[i0]
  float scale;      // equalize: 255 / (total - h[i0])
  bool identity;    // one value holds every entry (equalize), or hi <= lo (stretch)
};

// The stretch rule's cuts: (total * clip) >> 16 in 64 bits.
VF_LEVEL_FN uint64_t cut(uint64_t total, int clip) { return (total * (uint64_t)clip) >> 16; }

// The scalars from the two searches' results (each search is over running sums, so the host walks
// and the device counts ballots): lo = the smallest v with h[0] + .. + h[v] > cut_lo (cut_lo = 0
// for equalize: the first non-empty bin), hi = the largest v with h[v] + .. + h[255] > cut_hi,
// h_lo = h[lo].
VF_LEVEL_FN Scalars level_scalars(int rule, uint64_t total, uint32_t lo, uint32_t hi, uint32_t h_lo) {
  Scalars s;
  s.lo = lo;
  s.hi = hi;
  s.base = h_lo;
  s.scale = 0.f;
  if (rule == kEqualize) {
    s.identity = (uint64_t)h_lo == total;
    if (!s.identity) s.scale = VF_LEVEL_FDIV(255.0f, VF_LEVEL_U2F((uint32_t)(total - h_lo)));
  } else {
    s.identity = hi <= lo;
  }
  return s;
}

// table[v] from cum = h[0] + .. + h[v].
VF_LEVEL_FN uint32_t level_entry(int rule, const Scalars &s, uint32_t v, uint32_t cum) {
  if (s.identity) return v;
  if (v <= s.lo) return 0;
  if (rule == kEqualize) {
    // cum - h[i0] = h[i0 + 1] + .. + h[v]: bins below i0 are empty
    const int r = VF_LEVEL_F2I(VF_LEVEL_FMUL(VF_LEVEL_U2F(cum - s.base), s.scale));
    return (uint32_t)(r < 0 ? 0 : r > 255 ? 255 : r);
  }
  if (v >= s.hi) return 255;
  const uint32_t d = s.hi - s.lo;
  return (510u * (v - s.lo) + d) / (2u * d);  // round half up; at most 255
}

// The rule as one function: a histogram h of `total` entries (total >= 1, the sum of h, at most
// 2^32 - 1) to its table.  clip_lo and clip_hi are read by the stretch rule only.
VF_LEVEL_FN void level_table(const uint32_t h[256], uint64_t total, int rule, int clip_lo, int clip_hi,
                             uint8_t out[256]) {
  const uint64_t cut_lo = rule == kStretch ? cut(total, clip_lo) : 0;
  const uint64_t cut_hi = rule == kStretch ? cut(total, clip_hi) : 0;
  uint32_t lo = 0, hi = 255;
  uint64_t run = 0;
  for (uint32_t v = 0; v < 256; ++v) {
    run += h[v];
    if (run > cut_lo) {
      lo = v;
      break;
    }
  }
  run = 0;
  for (int v = 255; v >= 0; --v) {
    run += h[v];
    if (run > cut_hi) {
      hi = (uint32_t)v;
      break;
    }
  }
  const Scalars s = level_scalars(rule, total, lo, hi, h[lo]);
  uint64_t cum = 0;
  for (uint32_t v = 0; v < 256; ++v) {
    cum += h[v];
    out[v] = (uint8_t)level_entry(rule, s, v, (uint32_t)cum);
  }
}

// ---- limits (host) -----------------------------------------------------------------------------------

inline int mask_count(int mask) { return (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1); }

// The mask with 0 resolved to all of the frame's channels.
inline int resolved_mask(int mask, int channels) { return mask == 0 ? (1 << channels) - 1 : mask; }

// The filter arguments of every entry point and of a VF_STEP_LEVEL step; false with the reason in *why.
inline bool limits_ok(int rule, int mask, int link, int clip_lo, int clip_hi, int channels, std::string *why) {
  auto fail = [&](const std::string &m) {
    if (why) *why = m;
    return false;
  };
  if (rule != kEqualize && rule != kStretch) return fail("unknown level rule " + std::to_string(rule));
  if (channels != 1 && channels != 3) return fail("channels=" + std::to_string(channels) + ", a frame has 1 or 3");
  if (mask < 0 || mask > 7) return fail("channel mask " + std::to_string(mask) + " outside 0..7");
  if (mask >> channels)
    return fail("channel mask " + std::to_string(mask) + " names a channel beyond the frame's " + std::to_string(channels));
  if (link != 0 && link != 1) return fail("link=" + std::to_string(link) + " is not 0 or 1");
  if (clip_lo < 0 || clip_lo > kMaxClip || clip_hi < 0 || clip_hi > kMaxClip)
    return fail("clips " + std::to_string(clip_lo) + ", " + std::to_string(clip_hi) + " outside 0.." + std::to_string(kMaxClip));
  if (rule == kEqualize && (clip_lo != 0 || clip_hi != 0)) return fail("the equalize rule takes no clips; they must be 0");
  return true;
}

// A frame of `pixels` pixels under the limits: every bin, and with link the sum of the masked
// channels' bins, fits 32 bits.
inline bool pixels_ok(uint64_t pixels, int mask, int link, int channels, std::string *why) {
  if (pixels > kMaxPixels) {
    if (why) *why = "a frame of " + std::to_string(pixels) + " pixels; at most " + std::to_string(kMaxPixels);
    return false;
  }
  const uint64_t linked = pixels * (uint64_t)(link ? mask_count(resolved_mask(mask, channels)) : 1);
  if (linked > kMaxPixels) {
    if (why)
      *why = "linked channels of " + std::to_string(pixels) + " pixels sum to " + std::to_string(linked) + " entries; at most " +
             std::to_string(kMaxPixels);
    return false;
  }
  return true;
}

}  // namespace level
}  // namespace vf
