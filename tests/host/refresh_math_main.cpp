// Host driver for csrc/tld_refresh_math.h: the integer bf16 and e4m3 roundings of the device weight refresh against the host's own
// (f32_to_bf16_rne of csrc/tld_stages.h; e4m3_rne of csrc/tld_quant.hip, restated here through frexpf / lrintf as it is written there), on every
// `stride`-th fp32 bit pattern.  refresh_math_main [stride = 1: all 2^32 patterns, about half a minute].  Exit status 1 on any mismatch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tld_refresh_math.h"
#include "tld_stages.h"

namespace tld { void set_last_error(const char*) {} }

static uint8_t e4m3_reference(float f) {
    const uint8_t sign = std::signbit(f) ? 0x80 : 0;
    const float a = fabsf(f);
    if (!(a == a)) return sign | 0x7f;
    if (a >= 448.f) return sign | 0x7e;
    if (a < 0.015625f) return sign | (uint8_t)lrintf(a * 512.f);
    int e;
    const float m = frexpf(a, &e);
    int q = (int)lrintf(m * 16.f) - 8, ex = e - 1;
    if (q == 8) { q = 0; ex += 1; }
    if (ex > 8 || (ex == 8 && q > 6)) return sign | 0x7e;
    return sign | (uint8_t)(((ex + 7) << 3) | q);
}

int main(int argc, char** argv) {
    const unsigned long long stride = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    if (!stride) return 2;
    unsigned long long bad = 0, n = 0;
    for (unsigned long long u = 0; u < (1ull << 32); u += stride, ++n) {
        const uint32_t v = (uint32_t)u;
        float f;
        memcpy(&f, &v, 4);
        if (tld::e4m3_rne_bits(v) != e4m3_reference(f) && bad++ < 8) printf("e4m3 %08x: %02x, reference %02x\n", v, tld::e4m3_rne_bits(v), e4m3_reference(f));
        if (tld::bf16_rne_bits(v) != tld::f32_to_bf16_rne(f) && bad++ < 8) printf("bf16 %08x: %04x, reference %04x\n", v, tld::bf16_rne_bits(v), tld::f32_to_bf16_rne(f));
    }
    printf("%llu values, %llu mismatches\n", n, bad);
    return bad != 0;
}
