// tld_batch_math.h -- the random number generator of the device batch preparation (tld_batch.hip) and its bits-to-uniform
// conversions, one spelling for host and device: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) in plain
// integer arithmetic, and the conversions in operations that round the same everywhere.  No HIP in this file: tests/host/batch_math_main.cpp
// compiles it on its own and tests/batch_prep_ref.py restates it in numpy.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define TLD_HD __host__ __device__ __forceinline__
#else
#define TLD_HD inline
#endif

namespace tld {

// the counter's second word: 4 replica + stream
enum : uint32_t { BATCH_STREAM_NOISE = 0, BATCH_STREAM_LEVEL = 1, BATCH_STREAM_MASK = 2 };
// stream 1 (the Beta draw of sample b): c0 = BATCH_LEVEL_SLOTS b + slot.  Gamma(a) owns slots [0, 32), Gamma(b) slots [32, 64): attempt j of the
// rejection loop reads slot base + j, the boost uniform of a shape below 1 reads slot base + BATCH_GAMMA_TRIES.
constexpr uint32_t BATCH_LEVEL_SLOTS = 64;
constexpr int BATCH_GAMMA_TRIES = 16;

struct Philox4 { uint32_t v[4]; };

TLD_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// the counter of one draw: (c0, 4 replica + stream, step_lo, step_hi) under the key (seed_lo, seed_hi)
TLD_HD Philox4 batch_philox(uint64_t seed, uint64_t step, uint32_t replica, uint32_t stream, uint32_t c0) {
    return philox4x32_10(c0, 4u * replica + stream, (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// ((r >> 8) + 0.5) 2^-24 in fp32, in (0, 1]: never 0, so its logarithm is finite.  The sum is ONE fp32 addition: from r >> 8 = 2^23 on it has 25
// significant bits and rounds to even (up to 1.0 for the last code) -- part of the definition, the same on every host and device.
TLD_HD float uniform24_open(uint32_t r) { return ((float)(r >> 8) + 0.5f) * 5.9604644775390625e-8f; }

// 1 - ((r >> 8) + 0.5) 2^-24 as (2^24 - (r >> 8) - 0.5) 2^-24: EXACT in fp32 for r >> 8 >= 2^23, the half where uniform24_open has to round.  The radius
// of a normal takes ln u from log1p(-this) there: next to u = 1 the rounding of u itself (2^-25) would be an error of 2^-25 / radius in the radius.
TLD_HD float uniform24_open_complement(uint32_t r) { return ((float)(0x1000000u - (r >> 8)) - 0.5f) * 5.9604644775390625e-8f; }

// float(r >> 8) 2^-24 in [0, 1): exact
TLD_HD float uniform24(uint32_t r) { return (float)(r >> 8) * 5.9604644775390625e-8f; }

// 53 bits of (hi, lo) + 0.5, times 2^-53: a double in (0, 1]; k + 0.5 is exact for k < 2^52 and rounds to even above
// (up to 1.0 for the last code) -- again one addition, part of the definition
TLD_HD double uniform53_open(uint32_t hi, uint32_t lo) {
    const uint64_t k = (((uint64_t)hi << 32) | lo) >> 11;
    return ((double)k + 0.5) * 1.1102230246251565404e-16;
}

// (r + 0.5) 2^-32 as a double in (0, 1): exact
TLD_HD double uniform32_open(uint32_t r) { return ((double)r + 0.5) * 2.3283064365386962891e-10; }

}  // namespace tld
