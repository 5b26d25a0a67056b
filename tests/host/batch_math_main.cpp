// Host driver for csrc/tld_batch_math.h: the generator of the device batch preparation compiled by the host compiler alone.
// batch_math_main kat                          -> the three published Philox4x32-10 known answers, one line of four words each
// batch_math_main <seed> <step> <replica> <n>  -> for streams 0, 1, 2 and c0 = 0 .. n - 1, and for the same n counters ending at 2^32 - 1 on stream 0:
//                                                 the four words, then the bits of uniform24_open, uniform24, uniform24_open_complement (fp32) per word, uniform53_open(w0, w1) and
//                                                 uniform32_open(w2) (fp64) -- tests/test_batch_prep_host.py compares every field with numpy's
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tld_batch_math.h"

static uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static uint64_t dbits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

static void line(uint32_t stream, uint32_t c0, const tld::Philox4& p) {
    printf("%u %u", stream, c0);
    for (int i = 0; i < 4; ++i) printf(" %08x", p.v[i]);
    for (int i = 0; i < 4; ++i)
        printf(" %08x %08x %08x", fbits(tld::uniform24_open(p.v[i])), fbits(tld::uniform24(p.v[i])), fbits(tld::uniform24_open_complement(p.v[i])));
    printf(" %016" PRIx64 " %016" PRIx64 "\n", dbits(tld::uniform53_open(p.v[0], p.v[1])), dbits(tld::uniform32_open(p.v[2])));
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "kat")) {
        const uint32_t in[3][6] = {{0, 0, 0, 0, 0, 0},
                                   {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                                   {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
        for (const auto& t : in) {
            const tld::Philox4 p = tld::philox4x32_10(t[0], t[1], t[2], t[3], t[4], t[5]);
            printf("%08x %08x %08x %08x\n", p.v[0], p.v[1], p.v[2], p.v[3]);
        }
        return 0;
    }
    if (argc != 5) return 2;
    const uint64_t seed = strtoull(argv[1], nullptr, 0), step = strtoull(argv[2], nullptr, 0);
    const uint32_t replica = (uint32_t)strtoul(argv[3], nullptr, 0), n = (uint32_t)strtoul(argv[4], nullptr, 0);
    for (uint32_t stream = 0; stream < 3; ++stream)
        for (uint32_t c0 = 0; c0 < n; ++c0) line(stream, c0, tld::batch_philox(seed, step, replica, stream, c0));
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c0 = 0xffffffffu - i;
        line(0, c0, tld::batch_philox(seed, step, replica, 0, c0));
    }
    return 0;
}
