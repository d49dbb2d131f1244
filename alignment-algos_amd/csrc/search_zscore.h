// search_zscore.h — the pieces of aln_hits_zscores / aln_hits_zscores_profiles (search_zscore.hip) that are not kernels: the
// shuffle rule, stated once for the device and the host, the class of a hit slot, the z formula and the two budgets.
#pragma once
#include <algorithm>
#include <cmath>

#include "score_common.h"

namespace aln {

constexpr int kShufGroup = 32;                    // most shuffles one wave scores (template state is set up once per wave)
constexpr size_t kZBudget = (size_t)1 << 30;      // bytes of shuffled strings (or orders), and of accumulators, resident at a time

__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}

// Shuffle s of query q under `seed` (the rule of include/aln_hip.h): Fisher-Yates from the top over `interior`, what lies between
// the sentinels — residue codes on the device, residue characters on the host, or the indices 0 .. n-1 of a profile's interior
// rows — n of them.  Serial per string; the strings are independent.
template <class V>
__host__ __device__ __forceinline__ void shuffle_interior(uint32_t seed, uint32_t q, uint32_t s, V* interior, int n) {
  const uint32_t key = fmix32(fmix32(fmix32(seed ^ 0x9E3779B9u) + q) + s);
  for (int i = n - 1; i >= 1; --i) {
    const uint32_t r = fmix32(key + (uint32_t)i * 0x9E3779B9u);
    const int j = (int)(((uint64_t)r * (uint32_t)(i + 1)) >> 32);
    const V x = interior[i]; interior[i] = interior[j]; interior[j] = x;
  }
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

inline float z_of(int64_t n, float score, int64_t sum, int64_t sumsq) {
  if (n < 2) return 0.0f;
  const __int128 D = (__int128)n * sumsq - (__int128)sum * sum;
  if (D == 0) return 0.0f;
  const int64_t N = n * (int64_t)score - sum;
  return (float)((double)N * sqrt((double)(n - 1) / ((double)n * (double)D)));
}

}  // namespace aln
