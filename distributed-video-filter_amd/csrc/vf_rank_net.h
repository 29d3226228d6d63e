// vf_rank_net.h — the median selection networks of the rank filter (cv2.medianBlur, ksize 3 and
// 5): fixed sequences of compare-exchanges, lo = min(a, b), hi = max(a, b), independent of the
// data.  The kernel (vf_rank.hip) runs them on packed byte pairs and the CPU checker
// (tests/rank/rank_net_check.cc) proves them by the 0-1 principle; both compile this one text.
// Not installed.
//
// A network is a template over the element type T and an Ops class with
//   static T lo(T a, T b);   // the smaller of each element
//   static T hi(T a, T b);   // the larger
// An exchange whose one output nothing reads costs one operation, not two: the compiler drops
// the other (every loop here has constant bounds and is unrolled, so v[] stays in registers).
#pragma once

#if defined(__HIPCC__)
#define VF_RANK_HD __host__ __device__ __forceinline__
#else
#define VF_RANK_HD inline
#endif

namespace vf {
namespace rank {

// v[a] <- min, v[b] <- max
template <class Ops, class T, int N>
VF_RANK_HD void cx(T (&v)[N], int a, int b) {
  const T lo = Ops::lo(v[a], v[b]), hi = Ops::hi(v[a], v[b]);
  v[a] = lo;
  v[b] = hi;
}

// The median of 9: the 19-exchange network of Paeth (Graphics Gems, 1990) in Devillard's order.
// The median ends in v[4]; v is scratch.
constexpr int kMedian9Exchanges = 19;
template <class Ops, class T>
VF_RANK_HD T median9(T (&v)[9]) {
  constexpr int net[kMedian9Exchanges][2] = {{1, 2}, {4, 5}, {7, 8}, {0, 1}, {3, 4}, {6, 7}, {1, 2}, {4, 5}, {7, 8}, {0, 3},
                                             {5, 8}, {4, 7}, {3, 6}, {1, 4}, {2, 5}, {4, 7}, {4, 2}, {6, 4}, {4, 2}};
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int e = 0; e < kMedian9Exchanges; ++e) cx<Ops>(v, net[e][0], net[e][1]);
  return v[4];
}

// The smallest of v[lo..hi] to v[lo] and the largest to v[hi], everything else kept (in some
// order): neighbours pairwise, then the pairs' smaller ones against v[lo] and their larger ones
// against v[hi]; with an odd count the element without a partner goes against both.
template <class Ops, class T, int N>
VF_RANK_HD void min_max_to_ends(T (&v)[N], int lo, int hi) {
  const int m = hi - lo + 1, pairs = m / 2;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int p = 0; p < pairs; ++p) cx<Ops>(v, lo + p, hi - p);  // v[lo + p] <= v[hi - p]
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int p = 1; p < pairs; ++p) {
    cx<Ops>(v, lo, lo + p);
    cx<Ops>(v, hi - p, hi);
  }
  if (m & 1) {  // the middle element
    cx<Ops>(v, lo, lo + pairs);
    cx<Ops>(v, lo + pairs, hi);
  }
}

// The median of 25 by forgetful selection: of any 14 values the smallest has 13 that are not
// smaller and the largest 13 that are not larger, so neither is the 13th of 25; drop both, take
// in the next value, and the same holds for 13 of the rest with the two dropped, and so on until
// three are left, whose middle is the median.  Sets of 14, 13, ..., 3 values cost 19 + 18 + 16 +
// 15 + 13 + 12 + 10 + 9 + 7 + 6 + 4 + 3 = 132 exchanges (the checker counts them).  Devillard's
// table for 25 has 99; this one is generated and proven, not copied.
constexpr int kMedian25Exchanges = 132;
template <class Ops, class T>
VF_RANK_HD T median25(T (&v)[25]) {
  // the working set is v[lo..13]: 14 values at lo = 0; each step leaves v[lo] (the smallest) behind
  // and overwrites v[13] (the largest) with the next unseen value
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int step = 0; step < 12; ++step) {
    const int m = 14 - step, lo = step, hi = lo + m - 1;
    min_max_to_ends<Ops>(v, lo, hi);
    if (step < 11) v[hi] = v[14 + step];  // hi = 13 always: the set shrinks from below
  }
  return v[12];  // the last set was v[11..13]: its middle
}

}  // namespace rank
}  // namespace vf
