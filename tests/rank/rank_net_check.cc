// rank_net_check.cc — CPU proof of the median networks in csrc/vf_rank_net.h (built by
// tests/test_rank_net.py with -fsanitize=address,undefined).  The kernel compiles the same text.
//
// A network of compare-exchanges (lo = min, hi = max) computes the median of every input exactly
// when it does so for every input of zeros and ones (the 0-1 principle: min and max commute with
// every threshold x >= t).  So each network is run on ALL 2^9, respectively 2^25, zero/one inputs,
// 64 of them per uint64_t -- min is AND, max is OR -- and its output must be 1 exactly when at least
// 5 of 9, respectively 13 of 25, inputs are 1.  Each network then runs on 10^4 seeded random byte
// vectors (all-equal vectors and vectors of only 0 and 255 among them) against std::nth_element,
// and its exchanges are counted against the constants the header states.
// Prints one JSON object; exit status 0 when nothing failed.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "vf_rank_net.h"

struct BitOps {  // 64 zero/one inputs per word
  static uint64_t lo(uint64_t a, uint64_t b) { return a & b; }
  static uint64_t hi(uint64_t a, uint64_t b) { return a | b; }
};

static long g_lo_calls = 0;
struct ByteOps {
  static uint8_t lo(uint8_t a, uint8_t b) {
    ++g_lo_calls;  // one per exchange
    return a < b ? a : b;
  }
  static uint8_t hi(uint8_t a, uint8_t b) { return a < b ? b : a; }
};

template <int N>
struct Net;
template <>
struct Net<9> {
  template <class Ops, class T>
  static T run(T (&v)[9]) { return vf::rank::median9<Ops>(v); }
};
template <>
struct Net<25> {
  template <class Ops, class T>
  static T run(T (&v)[25]) { return vf::rank::median25<Ops>(v); }
};

// every zero/one input of N values: input x (its bit i is value i) is lane x % 64 of word x / 64
template <int N>
static uint64_t zero_one(uint64_t *failed) {
  const uint64_t words = N <= 6 ? 1 : (uint64_t)1 << (N - 6);
  uint64_t low[6];  // values 0..5 of the 64 inputs of any word
  for (int i = 0; i < 6; ++i) {
    low[i] = 0;
    for (int l = 0; l < 64; ++l)
      if ((l >> i) & 1) low[i] |= (uint64_t)1 << l;
  }
  uint64_t checked = 0;
  for (uint64_t b = 0; b < words; ++b) {
    uint64_t v[N];
    for (int i = 0; i < N; ++i) v[i] = i < 6 ? low[i] : ((b >> (i - 6)) & 1) ? ~(uint64_t)0 : 0;
    const int high_ones = __builtin_popcountll(b);
    uint64_t want = 0;
    for (int l = 0; l < 64; ++l)
      if (high_ones + __builtin_popcount((unsigned)l) >= N / 2 + 1) want |= (uint64_t)1 << l;
    const uint64_t got = Net<N>::template run<BitOps>(v);
    *failed += (uint64_t)__builtin_popcountll(got ^ want);
    checked += 64;
  }
  return checked;
}

static uint32_t g_seed = 0x9E3779B9u;
static uint32_t rnd() {
  g_seed = g_seed * 1664525u + 1013904223u;
  return g_seed >> 8;
}

template <int N>
static long random_bytes(int count, uint64_t *failed, long *exchanges) {
  for (int t = 0; t < count; ++t) {
    uint8_t v[N], s[N];
    const int kind = t % 4;  // 0, 1: any bytes; 2: all equal; 3: only 0 and 255
    const uint8_t same = (uint8_t)rnd();
    for (int i = 0; i < N; ++i) v[i] = kind == 2 ? same : kind == 3 ? ((rnd() & 1) ? 255 : 0) : (uint8_t)rnd();
    for (int i = 0; i < N; ++i) s[i] = v[i];
    std::nth_element(s, s + N / 2, s + N);
    g_lo_calls = 0;
    const uint8_t got = Net<N>::template run<ByteOps>(v);
    if (t == 0) *exchanges = g_lo_calls;
    else if (g_lo_calls != *exchanges) ++*failed;  // a network: the same exchanges whatever the data
    if (got != s[N / 2]) ++*failed;
  }
  return count;
}

int main() {
  uint64_t failed = 0;
  long ex9 = 0, ex25 = 0;
  const uint64_t z9 = zero_one<9>(&failed);
  const uint64_t z25 = zero_one<25>(&failed);
  const long r9 = random_bytes<9>(10000, &failed, &ex9);
  const long r25 = random_bytes<25>(10000, &failed, &ex25);
  if (ex9 != vf::rank::kMedian9Exchanges || ex25 != vf::rank::kMedian25Exchanges) ++failed;
  printf("{\"zero_one_9\": %llu, \"zero_one_25\": %llu, \"random_9\": %ld, \"random_25\": %ld, "
         "\"exchanges_9\": %ld, \"exchanges_25\": %ld, \"failed\": %llu}\n",
         (unsigned long long)z9, (unsigned long long)z25, r9, r25, ex9, ex25, (unsigned long long)failed);
  return failed ? 1 : 0;
}
