// vf_conv_border.h — where an out-of-range tap of the 2-D convolution filter reads (cv2.filter2D's
// border modes), one axis at a time.  The kernel (vf_conv.hip) and the CPU checker
// (tests/conv/conv_bands_check.cc) compile this one text.  Not installed.
#pragma once

#if defined(__HIPCC__)
#define VF_CONV_HD __host__ __device__ inline
#else
#define VF_CONV_HD inline
#endif

namespace vf {
namespace conv {

// the values of the C ABI's `border` argument (VF_BORDER_* in include/vfilter.h)
constexpr int kReflect101 = 0;  // cv2.BORDER_REFLECT_101 = BORDER_DEFAULT: gfedcb|abcdefgh|gfedcba
constexpr int kReplicate = 1;   // cv2.BORDER_REPLICATE:                    aaaaaa|abcdefgh|hhhhhhh
constexpr int kConstant = 2;    // cv2.BORDER_CONSTANT with value 0:        000000|abcdefgh|0000000

constexpr int kMaxK = 7;  // the largest kernel side

// The index on an axis of n >= 1 elements that tap position p reads, or -1 when the tap
// contributes 0 (kConstant outside the axis).  Always resolved in FRAME coordinates: a band of
// rows cut out of a frame passes the frame's n and the frame's p.
VF_CONV_HD int border_index(int p, int n, int border) {
  if (p >= 0 && p < n) return p;
  if (border == kConstant) return -1;
  if (border == kReplicate) return p < 0 ? 0 : n - 1;
  if (n == 1) return 0;
  // a 7-tap kernel on a 2-element axis reflects more than once
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
  return p;
}

}  // namespace conv
}  // namespace vf
