// search_zscore.h — what aln_hits_zscores (search_zscore.hip) and aln_hits_zscores_profiles (search_zscore_profile.hip) share:
// the shuffle rule on the device and once more on the host, the class of a hit slot, the z formula and the two budgets.
#pragma once
#include <algorithm>
#include <cmath>

#include "score_common.h"

namespace aln {

constexpr int kShufGroup = 32;                    // most shuffles one wave scores (template state is set up once per wave)
constexpr size_t kZBudget = (size_t)1 << 30;      // bytes of shuffled strings (or orders), and of accumulators, resident at a time

__device__ __forceinline__ uint32_t fmix32(uint32_t x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}

// slot (row * K + k) -> the length class of its template, 0: beyond 2048 columns (scored on the host side), -1: unused slot
// (class_list_kernel, score_common.h)
struct SlotClass {
  const int32_t* slot_t; const int64_t* toff;
  __device__ int operator()(int h) const {
    const int t = slot_t[h];
    if (t < 0) return -1;
    const int T = (int)(toff[t + 1] - toff[t]);
    return T > 2048 ? 0 : (T + 255) / 256;
  }
};

// The permutation once more, on the host: the full-build route's queries do not come from the device kernels.  `interior` is
// what lies between the sentinels (residue characters, or the indices 0 .. n-1 of a profile's interior rows), n of them.
inline uint32_t host_fmix(uint32_t h) {
  h = (h ^ (h >> 16)) * 0x85EBCA6Bu;
  h = (h ^ (h >> 13)) * 0xC2B2AE35u;
  return h ^ (h >> 16);
}
template <class V>
inline void host_shuffle_interior(uint32_t seed, uint32_t q, uint32_t s, V* interior, int64_t n) {
  const uint32_t golden = 0x9E3779B9u;
  const uint32_t key = host_fmix(host_fmix(host_fmix(seed ^ golden) + q) + s);
  for (int64_t hi = n - 1; hi > 0; --hi) {
    const uint64_t draw = host_fmix(key + (uint32_t)hi * golden);
    const int64_t lo = (int64_t)((draw * (uint64_t)(hi + 1)) >> 32);
    std::swap(interior[hi], interior[lo]);
  }
}
inline void host_shuffle(uint32_t seed, uint32_t q, uint32_t s, char* seq, int64_t Q) {
  host_shuffle_interior(seed, q, s, seq + 1, Q - 2);   // '^' and '$' stay
}

inline float z_of(int64_t n, float score, int64_t sum, int64_t sumsq) {
  if (n < 2) return 0.0f;
  const __int128 D = (__int128)n * sumsq - (__int128)sum * sum;
  if (D == 0) return 0.0f;
  const int64_t N = n * (int64_t)score - sum;
  return (float)((double)N * sqrt((double)(n - 1) / ((double)n * (double)D)));
}

}  // namespace aln
