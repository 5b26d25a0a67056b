// tld_refresh_math.h -- the two roundings of the weight images in integer form, one spelling for host and device: bf16 (f32_to_bf16_rne of tld_stages.h)
// and OCP e4m3 (e4m3_rne of tld_quant.hip).  The device weight refresh (tld_refresh.hip) must reproduce the bits tld_engine_finalize_weights computes
// on the host, so neither goes through a hardware convert.  No HIP in this file: tests/host/refresh_math_main.cpp compiles it on its own.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define TLD_HD __host__ __device__ __forceinline__
#else
#define TLD_HD inline
#endif

namespace tld {

// round-to-nearest-even to the upper 16 bits; a NaN stays a (quiet) NaN
TLD_HD uint16_t bf16_rne_bits(uint32_t u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// the e4m3 code of the fp32 value with bits u: saturating at +-448 (0x7e), NaN -> 0x7f, subnormals are multiples of 2^-9, everything
// round-to-nearest-even.  Normal range: the 23-bit mantissa is cut to 3 bits in place (a carry runs into the exponent), and the exponent is re-biased
// from 127 to 7.  Below 2^-6: the count of 2^-9 steps is at most 8, read off the fixed-point value of |v| 2^9 with its dropped bits.
TLD_HD uint8_t e4m3_rne_bits(uint32_t u) {
    const uint8_t sign = (uint8_t)((u >> 24) & 0x80u);
    const uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return sign | 0x7f;
    if (a >= 0x43e00000u) return sign | 0x7e;                  // |v| >= 448
    if (a >= 0x3c800000u) {                                    // |v| >= 2^-6: normal codes
        const uint32_t r = a + 0x7ffffu + ((a >> 20) & 1u);
        return sign | (uint8_t)((r >> 20) - ((127u - 7u) << 3));
    }
    const int e = (int)(a >> 23);                              // biased exponent < 121: |v| 2^9 = m 2^(e - 141), m the 24-bit significand, is below 8
    const uint32_t m = (a & 0x7fffffu) | 0x800000u;
    const int sh = 141 - e;                                    // dropped bits, 21 or more
    if (sh > 25) return sign;                                  // m < 2^24 is below half a step (fp32 subnormals, e = 0, are far below)
    const uint32_t q = m >> sh, rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
    return sign | (uint8_t)(q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));
}

// Row of the pair-ordered QKV weight image (qkv_wp2, EPI_QKV_ATTN2) that holds row r (0 .. 63) of (part = q | k | v, head): a 256 x 384 tile is the head pair
// head >> 1, its columns [wave column = feature / 16][part][side = head & 1][16 features] -- every 96-column wave tile holds 16 features of q, k and v of both heads
TLD_HD int qkv_pair_row(int part, int head, int r) {
    return (head >> 1) * 384 + (r >> 4) * 96 + part * 32 + (head & 1) * 16 + (r & 15);
}

}  // namespace tld
