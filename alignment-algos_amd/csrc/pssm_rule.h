// pssm_rule.h — the exact log-odds rule of aln_hits_pssm (include/aln_hip.h has the definition), for host and device.
//
// One score is round(scale * log2(num / den)) made of integers alone: lg16(x, y) is floor(16 * log2(x / y)) read off a 33-bit
// mantissa of x / y against the fifteen constants T[m] = floor(2^(32 + m/16)), and the score rounds lg16 * scale / 16 to the
// nearest integer.  No 128-bit arithmetic and no 64-bit division: the mantissa is one subtraction and 32 shift-and-subtract
// steps.  x and y are in [1, 2^63), so y * 2^e <= x < 2^63 and twice a remainder, below 2 * y * 2^e, never leaves 64 bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ALN_PSSM_HD __host__ __device__ __forceinline__
#else
#define ALN_PSSM_HD inline
#endif

namespace aln {

// the low 32 bits of T[1] .. T[15] (every T[m] is in [2^32, 2^33): bit 32 is set in all of them, as it is in the mantissa)
ALN_PSSM_HD uint32_t pssm_t_low(int m) {
  switch (m) {
    case 1: return 0x0b5586cfu; case 2: return 0x172b83c7u; case 3: return 0x2387a6e7u; case 4: return 0x306fe0a3u;
    case 5: return 0x3dea64c1u; case 6: return 0x4bfdad53u; case 7: return 0x5ab07dd4u; case 8: return 0x6a09e667u;
    case 9: return 0x7a11473eu; case 10: return 0x8ace5422u; case 11: return 0x9c49182au; case 12: return 0xae89f995u;
    case 13: return 0xc199bdd8u; case 14: return 0xd5818dcfu; default: return 0xea4afa2au;
  }
}

ALN_PSSM_HD int pssm_clz64(uint64_t v) { return __builtin_clzll(v); }   // v >= 1

// lg16(x, y) for 2^63 > x >= y >= 1
ALN_PSSM_HD int pssm_lg16(uint64_t x, uint64_t y) {
  int e = pssm_clz64(y) - pssm_clz64(x);                // y << e has x's bit length: the largest e, or one beyond it
  if ((y << e) > x) --e;
  const uint64_t d = y << e;                            // d <= x < 2 d
  uint64_t r = x - d;
  uint32_t frac = 0;                                    // mant = 2^32 + frac, frac = floor(r 2^32 / d)
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    r <<= 1;                                            // r < d before, so 2 r < 2 d < 2^64
    const bool bit = r >= d;
    r -= bit ? d : 0;
    frac = (frac << 1) | (bit ? 1u : 0u);
  }
  int below = 0;
#pragma unroll
  for (int m = 1; m <= 15; ++m) below += pssm_t_low(m) <= frac ? 1 : 0;
  return 16 * e + below;
}

// the score of num / den in 1 / scale bits; num and den in [1, 2^63), scale one of 1, 2, 4, 8
ALN_PSSM_HD int32_t pssm_score(uint64_t num, uint64_t den, int32_t scale) {
  const bool up = num >= den;                           // one lg16 either way: the lanes of a wave do not part
  const int32_t s = (pssm_lg16(up ? num : den, up ? den : num) * scale + 8) >> 4;
  return up ? s : -s;
}

ALN_PSSM_HD bool pssm_scale_ok(int32_t scale) { return scale == 1 || scale == 2 || scale == 4 || scale == 8; }

}  // namespace aln
